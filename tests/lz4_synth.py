"""Sequence-level LZ4 stream builder (TEST CODE ONLY).

A frame is a list of blocks, each one of
  ("stored", data)                  a stored (uncompressed) block, may be empty;
  ("seq", [(lits, off, ml), ...])   an LZ4 block: every sequence but the last has a match (offset `off`, length
                                    `ml` >= 4); the last one is `(lits, 0, 0)`, literals only;
  ("raw", body, stored_flag)        any block bytes, for malformed input the sequence list cannot express.
The builder writes the block bytes (exact 15 / 255 length encoding), the LZ4F frame around them with every header
choice, and the optional 12-byte lz4-mt skippable record.  `content()` decodes the sequence list the plain sequential
way, which is the reference the decoders under test are compared with: it shares no code with any of them.
"""
import ctypes as C
import hashlib
import os
import random
import struct

import xxhash

LZ4F_MAGIC = 0x184D2204
SKIP_MAGIC = 0x184D2A50


def _varlen(n):
    """the 255-continuation bytes of a length whose nibble is 15 (n = length - 15)"""
    return b"\xff" * (n // 255) + bytes([n % 255])


def seq_bytes(lits, off, ml, last=False):
    """one sequence: token, literal-length bytes, literals, then (unless last) offset and match-length bytes"""
    L = len(lits)
    ln = 15 if L >= 15 else L
    if last:
        mn = 0
    else:
        assert ml >= 4 and 0 <= off <= 0xFFFF
        mn = 15 if ml - 4 >= 15 else ml - 4
    out = bytearray([ln << 4 | mn])
    if ln == 15:
        out += _varlen(L - 15)
    out += lits
    if not last:
        out += struct.pack("<H", off)
        if mn == 15:
            out += _varlen(ml - 4 - 15)
    return bytes(out)


def block_body(seqs):
    """LZ4 block bytes of a sequence list whose last entry is (lits, 0, 0)"""
    out = bytearray()
    for i, (lits, off, ml) in enumerate(seqs):
        out += seq_bytes(lits, off, ml, last=(i == len(seqs) - 1))
    return bytes(out)


def decode_seqs(seqs, hist: bytearray, low: int):
    """append what `seqs` decode to onto `hist`; matches may reach back to hist[low].  Raises on a bad offset."""
    for i, (lits, off, ml) in enumerate(seqs):
        hist += lits
        if i == len(seqs) - 1:
            break
        if off == 0 or off > len(hist) - low:
            raise ValueError("offset %d outside the output (%d bytes)" % (off, len(hist) - low))
        s = len(hist) - off
        for j in range(ml):
            hist.append(hist[s + j])


def content(blocks, indep=False):
    """the decoded content of a frame, sequentially (None if a block is raw: it has no sequence list)"""
    out = bytearray()
    for b in blocks:
        if b[0] == "stored":
            out += b[1]
        elif b[0] == "seq":
            decode_seqs(b[1], out, len(out) if indep else 0)
        else:
            return None
    return bytes(out)


def frame(blocks, indep=False, csize=True, ccheck=True, bcheck=False, dict_id=None, bd=4, content_size=None,
          cchk_value=None, endmark=True):
    """LZ4F frame of `blocks`.  csize: write the content-size field (content_size overrides its value);
    cchk_value overrides the content checksum"""
    try:
        data = content(blocks, indep)
    except ValueError:
        data = None                     # a malformed sequence list: the header states its nominal size
    nominal = sum(len(b[1]) if b[0] == "stored" else sum(len(l) + m for l, _, m in b[1]) if b[0] == "seq" else 0
                  for b in blocks)
    flg = 0x40 | (0x20 if indep else 0) | (0x10 if bcheck else 0) | (0x08 if csize else 0) | \
        (0x04 if ccheck else 0) | (0x01 if dict_id is not None else 0)
    desc = bytes([flg, bd << 4])
    if csize:
        desc += struct.pack("<Q", content_size if content_size is not None else
                            len(data) if data is not None else nominal)
    if dict_id is not None:
        desc += struct.pack("<I", dict_id)
    out = bytearray(struct.pack("<I", LZ4F_MAGIC) + desc)
    out.append((xxhash.xxh32(desc, seed=0).intdigest() >> 8) & 0xFF)
    for b in blocks:
        if b[0] == "stored":
            body, stored = b[1], True
        elif b[0] == "seq":
            body, stored = block_body(b[1]), False
        else:
            body, stored = b[1], b[2]
        out += struct.pack("<I", len(body) | (0x80000000 if stored else 0)) + body
        if bcheck:
            out += struct.pack("<I", xxhash.xxh32(body, seed=0).intdigest())
    if endmark:
        out += b"\0\0\0\0"
    if ccheck:
        v = cchk_value if cchk_value is not None else xxhash.xxh32(data or b"", seed=0).intdigest()
        out += struct.pack("<I", v)
    return bytes(out)


def record(fr: bytes) -> bytes:
    """lz4-mt skippable record: magic, 4, frame size, frame"""
    return struct.pack("<III", SKIP_MAGIC, 4, len(fr)) + fr


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


# ------------------------------------------------------------------------------------------------------------------
# liblz4's verdict (the image's liblz4 1.9.3; what the reference calls per record)
_lz = None


def liblz4_path():
    return next((p for p in ("/opt/conda/lib/liblz4.so.1", "/usr/lib/x86_64-linux-gnu/liblz4.so.1")
                 if os.path.exists(p)), None)


def liblz4_decompress(fr: bytes, cap: int = 1 << 23):
    """LZ4F_decompress over the whole frame -> (accepted, content bytes).  Accepted = no error code and the frame fully
    consumed (return value 0: LZ4F has nothing more to read).  None if liblz4 is not on this machine."""
    global _lz
    path = liblz4_path()
    if path is None:
        return None
    if _lz is None:
        L = C.CDLL(path)
        L.LZ4F_createDecompressionContext.restype = C.c_size_t
        L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        L.LZ4F_freeDecompressionContext.restype = C.c_size_t
        L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
        L.LZ4F_decompress.restype = C.c_size_t
        L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                                      C.POINTER(C.c_size_t), C.c_void_p]
        L.LZ4F_isError.restype = C.c_uint
        L.LZ4F_isError.argtypes = [C.c_size_t]
        _lz = L
    ctx = C.c_void_p()
    assert not _lz.LZ4F_isError(_lz.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        dst = C.create_string_buffer(max(cap, 1))
        src = C.create_string_buffer(fr, len(fr))
        dn, sn = C.c_size_t(cap), C.c_size_t(len(fr))
        rv = _lz.LZ4F_decompress(ctx, dst, C.byref(dn), src, C.byref(sn), None)
        ok = (not _lz.LZ4F_isError(rv)) and rv == 0 and sn.value == len(fr)
        return ok, (dst.raw[:dn.value] if ok else None)
    finally:
        _lz.LZ4F_freeDecompressionContext(ctx)


# ------------------------------------------------------------------------------------------------------------------
# Stream families aimed at the decoders' thresholds.  Each case: name -> dict(frame, content (what the sequence list
# decodes to; None if it cannot be decoded), status (GPUMT_ST_* expected of every device variant when rejected, 0 when accepted, None when liblz4's
# verdict decides)).  Seeded and
# deterministic; where a family's condition follows from output positions alone it is asserted here, so a family
# cannot quietly stop covering its path.
ST_OK, ST_BAD_BLOCK, ST_SIZE_MISMATCH = 0, 3, 4
RINGS = (4096, 8192, 16384)


def _positions(seqs, op=0):
    """(output position of each sequence's literals, of its match) for one block starting at output `op`"""
    out = []
    for lits, off, ml in seqs:
        out.append((op, op + len(lits)))
        op += len(lits) + ml
    return out


def _tokens(seqs):
    """input position of every token of a block"""
    pos, at = [], 0
    for i, (lits, off, ml) in enumerate(seqs):
        pos.append(at)
        at += len(seq_bytes(lits, off, ml, last=(i == len(seqs) - 1)))
    return pos


C3_CSTAGE, C3_XOUT = 976, 2048   # lz4_dec_copy3.hip: the compressed-byte stage, the most output bytes of one batch


def copy3_first_batch(seqs, al, win=4096, o0=0):
    """The cut of the first batch of a block by copy3's rule (lz4_dec_copy3.hip, "cut"), restated: lane i looks at
    sequence i; its token sits at stage offset qr = (token position) + al, al = the block's address modulo 16.  A lane
    is small if its token's first bytes are staged (qr <= C3_CSTAGE - 12), its offset too (mo <= C3_CSTAGE - 4), no
    run is above 64 and it is not the block's last.  The batch is the run of small lanes whose output ends at most
    C3_XOUT past o0 and not past the ring lap.  -> dict(n = sequences in the batch, why = what cut it, qr, mo,
    ends = output end of every lane of the run, o_end)"""
    body, tok = block_body(seqs), _tokens(seqs)
    rem = len(seqs)
    qr, mo, small, v1s, v2s, bigs, lens = [], [], [], [], [], [], []
    for i in range(min(64, rem)):
        t, q = body[tok[i]], tok[i] - tok[0] + al
        lx, mx = (t >> 4) == 15, (t & 15) == 15
        lit = (t >> 4) + (body[tok[i] + 1] if lx else 0)
        m = q + 1 + (1 if lx else 0) + lit
        v1 = q <= C3_CSTAGE - 12
        v2 = v1 and m <= C3_CSTAGE - 4
        last = i + 1 == rem
        ml = 0 if last else (t & 15) + 4 + (body[tok[i] + 1 + (1 if lx else 0) + lit + 2] if mx else 0)
        big = 0xFFFF if last else max(lit, ml if v2 else 0)
        qr.append(q)
        mo.append(m)
        v1s.append(v1)
        v2s.append(v2)
        bigs.append(big)
        small.append(v2 and big <= 64)
        lens.append(lit + ml)
    n0 = next((i for i, x in enumerate(small) if not x), len(small))
    lap_end = (o0 | (win - 1)) + 1
    olim = min(o0 + C3_XOUT, lap_end)
    ends, op = [], o0
    for i in range(n0):
        op += lens[i]
        ends.append(op)
    n = next((i for i, e in enumerate(ends) if e > olim), n0)
    if n < n0:
        why = "xout" if olim == o0 + C3_XOUT else "lap"
    elif n0 == 64:
        why = "lanes"
    elif not v1s[n0]:
        why = "stage_tok"
    elif not v2s[n0]:
        why = "stage_off"
    else:
        why = "big"
    return {"n": n, "why": why, "qr": qr, "mo": mo, "ends": ends, "o_end": ends[n - 1] if n else o0}


class _Fam:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.cases = {}

    def lits(self, n):
        # text-like bytes: mostly a small alphabet, so an accidental repeat is harmless (the decoders do not care)
        return bytes(self.rng.choice(b"abcdefghijklmnopqrstuvwxyz ,.ETAOIN") for _ in range(n))

    def add(self, name, blocks, status=ST_OK, **fk):
        assert name not in self.cases, name
        indep = fk.get("indep", False)
        try:
            data = content(blocks, indep)
        except ValueError:
            data = None
        fr = frame(blocks, **fk)
        self.cases[name] = {"frame": fr, "content": data, "status": status}


def families(seed=1):
    F = _Fam(seed)
    L = F.lits
    tail = lambda: (L(8), 0, 0)

    # ---- literal runs: short, at the 15 / 255 length-byte edges, the 64 batch limit, the 976-byte stage ----
    for n in (0, 1, 14, 15, 16, 63, 64, 65, 269, 270, 271, 976, 977, 1500, 2100):
        F.add("lit_%d" % n, [("seq", [(L(16), 8, 4), (L(n), 16, 6), (L(n), 3, 5), tail()])])
    # ---- match lengths ----
    for m in (4, 18, 19, 20, 64, 65, 68, 272, 273, 274, 5000):
        F.add("ml_%d" % m, [("seq", [(L(120), 100, m), (L(2), 16, m), (L(0), 1, m), tail()])])
    # ---- offsets: 1-17 overlapping (offset < length), 63-65, every ring size -1/0/+1, 65535 ----
    base = L(70000)
    for o in list(range(1, 18)) + [63, 64, 65] + [r + d for r in RINGS for d in (-1, 0, 1)] + [65535]:
        for ml in ((3 * o + 5, 4) if o < 17 else (4, 40)):
            assert o >= 17 or ml == 4 or o < ml
            if o > 16000:   # far offsets: a 64 KiB stored block in front (sources in memory, not in the ring)
                blocks = [("stored", base[:65536]), ("seq", [(L(5), o, ml), (L(3), o, 64), tail()])]
            else:
                blocks = [("seq", [(base[:o + 20], o, ml), (L(1), o, ml), (L(7), o, 20), tail()])]
            F.add("off_%d_ml%d" % (o, ml), blocks)
    # offset 1 and 65535 over a whole 64 KiB block behind a stored block
    for o in (1, 65535):
        seqs = [(L(4), o, 65536 - 4 - 12), (L(12), 0, 0)]
        F.add("off_%d_full_block" % o, [("stored", base[:65536]), ("seq", seqs)])
    # ---- more than 64 small sequences; batches ending at and just past 2048 output bytes ----
    seqs = [(L(3), 3 + i % 29, 5 + i % 7) for i in range(300)]
    F.add("small_300", [("seq", [(L(40), 8, 4)] + seqs + [tail()])])
    for extra in (0, 1):
        # little input per output byte (8 bytes for 64), so the 2048-byte output limit cuts the block's first batch
        # before the stage and the 64 lanes do: at exactly 2048 (32 sequences), or one sequence early when the 32nd
        # would end at 2049
        seqs = [(L(4), 4, 60 + extra)] + [(L(4), 64, 60)] * 40 + [tail()]
        for win in RINGS:
            for al in range(16):
                b = copy3_first_batch(seqs, al, win)
                assert b["why"] == "xout", (extra, win, al, b["why"])
                assert (b["n"], b["o_end"]) == ((32, 2048) if extra == 0 else (31, 1985)), (b["n"], b["o_end"])
                assert extra == 0 or b["ends"][31] == 2049
        F.add("batch_2048_%d" % extra, [("seq", seqs)])
    # ---- small sequences across every multiple of 4 / 8 / 16 KiB ----
    for r in RINGS:
        for k in range(3):
            head = L(r - 7 - k * 2)
            seqs = [(head, 19, 4)] + [(L(3 + (i % 5)), 11 + i % 40, 6 + (i % 9)) for i in range(2000)] + [tail()]
            pos = _positions(seqs)
            ends = [(op, mp + ml) for (op, mp), (_, _, ml) in zip(pos, seqs)]
            assert any(a < r < b for a, b in ends[1:]), "no small sequence crosses %d" % r
            F.add("lap_%d_%d" % (r, k), [("seq", seqs)])
    # ---- the stage cuts the batch (copy3_first_batch): the first sequence left out has its token or its offset at
    # stage offsets 960 .. 976, for every alignment of the block (16-byte sequences, 17 output bytes: neither the 64 lanes nor the
    # output limit bind first) ----
    hit_tok, hit_off, last_in = set(), set(), set()
    for pad in range(16):
        seqs = [(L(13 + pad), 8, 4)] + [(L(13), 8, 4)] * 80 + [tail()]
        for al in range(16):
            b = copy3_first_batch(seqs, al)
            n = b["n"]
            assert b["why"] in ("stage_tok", "stage_off") and n < 64, (pad, al, b["why"])
            edge = range(C3_CSTAGE - 16, C3_CSTAGE + 1)
            assert b["qr"][n] in edge or b["mo"][n] in edge, (pad, al, b["qr"][n], b["mo"][n])
            assert b["mo"][n - 1] <= C3_CSTAGE - 4 < b["mo"][n], (pad, al)
            (hit_tok if b["why"] == "stage_tok" else hit_off).add(b["qr"][n] if b["why"] == "stage_tok" else b["mo"][n])
            last_in.update((("tok", b["qr"][n - 1]), ("off", b["mo"][n - 1])))
        F.add("stage_pad%d" % pad, [("seq", seqs)])
    # both bounds bind exactly at their edge: a token at C3_CSTAGE - 11 or an offset at C3_CSTAGE - 3 is left out, an
    # offset at C3_CSTAGE - 4 is the batch's last
    assert min(hit_tok) == C3_CSTAGE - 11 and min(hit_off) == C3_CSTAGE - 3, (sorted(hit_tok), sorted(hit_off))
    assert ("off", C3_CSTAGE - 4) in last_in
    # ---- stored blocks: matches into them, across their start and end; stored -> stored; empty ones ----
    s1, s2 = L(3000), L(700)
    F.add("stored_then_seq", [("seq", [(L(200), 50, 30), tail()]), ("stored", s1),
                              ("seq", [(L(4), 3004, 40), (L(2), 30, 60), (L(1), 10, 40), tail()])])
    F.add("stored_straddle", [("seq", [(L(300), 50, 30), tail()]), ("stored", s1),
                              ("seq", [(L(1), 3000 + 20, 64), (L(0), 80, 64), (L(3), 3000 + 330, 200), tail()])])
    F.add("stored_stored_seq", [("stored", s1), ("stored", s2), ("seq", [(L(3), 710, 64), (L(1), 3703, 30), tail()])])
    F.add("stored_empty_only", [("stored", b"")])
    F.add("stored_empty_first", [("stored", b""), ("seq", [(L(30), 20, 40), tail()])])
    F.add("stored_empty_mid", [("seq", [(L(30), 20, 40), tail()]), ("stored", b""), ("stored", s2),
                               ("stored", b""), ("seq", [(L(2), 100, 40), tail()])])
    F.add("stored_empty_last", [("seq", [(L(30), 20, 40), tail()]), ("stored", b"")])
    F.add("stored_empty_indep", [("stored", b""), ("seq", [(L(30), 20, 40), tail()]), ("stored", b"")], indep=True)
    # ---- linked blocks reaching into the previous one; independent blocks valid within each ----
    full = [(L(100), 90, 65536 - 100 - 12), (L(12), 0, 0)]
    F.add("linked_prev", [("seq", full), ("seq", [(L(3), 70, 100), (L(5), 65000, 64), tail()])])
    F.add("indep_blocks", [("seq", full), ("seq", [(L(30), 25, 100), tail()])], indep=True)
    # ---- blocks shorter than the maximum; more blocks than ceil(content / 64 KiB) ----
    F.add("short_blocks", [("seq", [(L(500), 100, 300), tail()])] * 5 + [("stored", L(100))])
    F.add("short_blocks_indep", [("seq", [(L(500), 100, 300), tail()])] * 5, indep=True)
    F.add("short_then_full", [("seq", [(L(40), 10, 20), tail()]), ("seq", full), ("seq", [(L(9), 9, 9), tail()])])
    # ---- frame header choices: BD 5/6/7, block checksums, dictionary id, no content size / checksum ----
    big = [(L(300), 250, 70000), (L(50), 60000, 200000), (L(20), 8, 9), tail()]
    for bd in (5, 6, 7):
        F.add("bd%d" % bd, [("seq", big if bd > 5 else big[:1] + [tail()])], bd=bd)
        F.add("bd%d_nocsize" % bd, [("seq", [(L(300), 250, 20000), tail()])], bd=bd, csize=False)
    F.add("bcheck", [("seq", [(L(30), 20, 40), tail()]), ("stored", s2), ("stored", b"")], bcheck=True)
    F.add("dictid", [("seq", [(L(30), 20, 40), tail()])], dict_id=0x12345678)
    F.add("nocsize", [("seq", [(L(100), 90, 30000), (L(12), 0, 0)])] * 2, csize=False)
    F.add("nocsize_nocheck", [("seq", [(L(90), 9, 900), tail()])], csize=False, ccheck=False)
    F.add("nocheck_indep", [("seq", [(L(90), 9, 900), tail()])], ccheck=False, indep=True)

    # ======================= malformed =======================
    B = ST_BAD_BLOCK
    F.add("bad_offset0", [("seq", [(L(30), 0, 8), tail()])], B)
    F.add("bad_offset_past_start", [("seq", [(L(30), 31, 8), tail()])], B)
    F.add("bad_offset_past_start_later", [("seq", [(L(30), 20, 40), tail()]), ("seq", [(L(3), 82, 8), tail()])], B,
          indep=False)
    F.add("ok_offset_at_start_later", [("seq", [(L(30), 20, 40), tail()]), ("seq", [(L(3), 81, 8), tail()])])
    F.add("bad_offset_across_indep", [("seq", [(L(30), 20, 40), tail()]), ("seq", [(L(3), 4, 8), tail()]),
                                      ("seq", [(L(3), 5, 8), tail()])], B, indep=True)
    F.add("bad_offset_far_after_stored", [("stored", s1), ("seq", [(L(3), 3004, 8), tail()])], B)
    body = block_body([(L(30), 20, 40), tail()])
    F.add("bad_lits_past_end", [("raw", body[:-3], False)], B, ccheck=False, content_size=64)
    F.add("bad_lits_past_end2", [("raw", bytes([0x80]) + L(7), False)], B, ccheck=False, content_size=64)
    F.add("bad_varint_lit_off_end", [("raw", bytes([0xF0]) + b"\xff" * 20, False)], B, ccheck=False, content_size=64)
    F.add("bad_varint_ml_off_end", [("raw", bytes([0x5F]) + L(5) + b"\x04\x00" + b"\xff" * 9, False)], B,
          ccheck=False, content_size=64)
    F.add("bad_ends_in_match", [("raw", bytes([0x50]) + L(5) + b"\x04\x00", False)], B, ccheck=False, content_size=64)
    F.add("bad_ends_in_offset", [("raw", bytes([0x50]) + L(5) + b"\x04", False)], B, ccheck=False, content_size=64)
    F.add("bad_past_64k", [("seq", [(L(100), 90, 65536 - 100 - 8), (L(12), 0, 0)])], B)
    F.add("bad_lits_past_64k", [("seq", [(L(100), 90, 65536 - 100 - 50), (L(51), 0, 0)])], B)
    F.add("bad_past_csize", [("seq", [(L(100), 90, 1000), tail()])], B, content_size=1000)   # (output overrun)
    F.add("bad_short_of_csize", [("seq", [(L(100), 90, 1000), tail()])], ST_SIZE_MISMATCH, content_size=1200)
    F.add("bad_block_above_max", [("raw", block_body([(L(65537 - 9), 0, 0)]), False)], B, ccheck=False)
    F.add("bad_stored_above_max", [("raw", L(65537), True)], B, ccheck=False)
    F.add("stored_empty_endmark", [("stored", b"")], ccheck=False, csize=False)
    # end of block (liblz4 1.9.3): last-sequence literal counts 0-5, the last match starting 11-13 bytes before the
    # end, in a block that fills its 64 KiB and in a short one.  Verdicts come from liblz4 (the manifest), the
    # sequence lists from here
    for fill in (True, False):
        for nl in range(6):
            for lm in (4, 8, 14, 15, 20):
                n = 65536 if fill else 3000
                seqs = [(L(100), 90, n - 100 - lm - nl - 3), (L(3), 50, lm), (L(nl), 0, 0)]
                F.add("eob_%s_last%d_m%d" % ("full" if fill else "short", nl, lm), [("seq", seqs)], None)
        for back in (11, 12, 13):
            # the last match starts `back` output bytes before the block's end: lit 0, match back - nl, nl literals
            for nl in (1, 5, 7):
                n = 65536 if fill else 3000
                seqs = [(L(100), 90, n - 100 - back), (L(0), 8, back - nl), (L(nl), 0, 0)]
                F.add("eob_%s_back%d_l%d" % ("full" if fill else "short", back, nl), [("seq", seqs)], None)
        for nl in range(4):
            for mlx in (14, 15, 300):
                # the previous sequence's literals (a run above 14 takes liblz4's checked path) end close to the end
                n = 65536 if fill else 3000
                seqs = [(L(100), 90, n - 100 - mlx - 6 - nl - 4), (L(mlx), 16, 6), (L(0), 9, 4), (L(nl), 0, 0)]
                F.add("eob_%s_lit%d_l%d" % ("full" if fill else "short", mlx, nl), [("seq", seqs)], None)
    return F.cases
