"""Helpers of the block-parallel record path tests (TEST CODE ONLY): batches of lz4-mt records through
gpumt_lz4_decompress_batch_par and through gpumt_lz4_decompress_batch, on the emulator and on the device, and the cases
that tests/test_emu_lz4_rec_par.py and tests/test_gpu_lz4_rec_par.py share.  A record is 12 bytes of
50 2A 4D 18 | 04 00 00 00 | csize followed by one LZ4 frame."""
import contextlib
import ctypes as C
import functools
import json
import os
import struct
import tempfile

import numpy as np

import emu_driver as E
import helpers as H
import lz4_blocks as LB
import lz4_seg as G
import lz4_synth as S
from golden import cases

CANARY = 0xCC
GAP = 7            # canary bytes between two records' output ranges (odd: the ranges start at every alignment)
JUNK = b"\xEE" * 3  # bytes between two records of the stream, which belong to no record
ST_OK, ST_BAD_RECORD, ST_BAD_FRAME, ST_BAD_BLOCK, ST_SIZE_MISMATCH, ST_BAD_CHECKSUM, ST_TRAILING = range(7)
KNOBS = dict(min_blocks=2, slice_blocks=4096, rec_par=1, seg=0, seg_bytes=65536, cap_mb=0)
DEFAULT_MIN_BLOCKS = 4096
TAIL = b"0123456789ab"
REC_MANIFEST = os.path.join(H.GOLDEN_DIR, "lz4_synth", "rec_manifest.json")


class Batch:
    """records = [(record bytes, out_len on entry (the content size, or a capacity))]"""

    def __init__(self, records, lead=0):
        self.records = [(bytes(r), int(c)) for r, c in records]
        n = len(self.records)
        self.rec_off, self.rec_len = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self.out_off, self.cap = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        stream, at = bytearray(JUNK + b"\xEE" * lead), GAP + lead
        for i, (r, c) in enumerate(self.records):
            self.rec_off[i], self.rec_len[i] = len(stream), len(r)
            stream += r + JUNK
            self.out_off[i], self.cap[i] = at, c
            at += c + GAP
        self.stream, self.out_bytes = bytes(stream), at

    def __len__(self):
        return len(self.records)


class Result:
    def __init__(self, batch, area, out_len, status, rec_par=None, stats=None):
        self.batch, self.area, self.out_len, self.status = batch, area, out_len, status
        self.rec_par, self.stats = rec_par, stats

    def bytes_of(self, i, n=None):
        o = int(self.batch.out_off[i])
        return self.area[o:o + int(self.out_len[i] if n is None else n)].tobytes()

    def gaps_intact(self):
        """every byte outside the records' [out_off, out_off + cap) still holds the canary"""
        keep = np.ones(len(self.area), bool)
        for o, c in zip(self.batch.out_off, self.batch.cap):
            keep[int(o):int(o) + int(c)] = False
        return bool((self.area[keep] == CANARY).all())


def _arrays(b):
    sbuf = np.frombuffer(b.stream + b"\xEE" * 320, np.uint8).copy()       # the device contract: 256 readable bytes behind
    area = np.full(b.out_bytes + 64, CANARY, np.uint8)
    return sbuf, area, b.rec_off.copy(), b.rec_len.copy(), b.out_off.copy(), b.cap.copy(), np.full(len(b), 99, np.uint32)


def emu_serial(b, variant=0):
    L = E.lib()
    sbuf, area, ro, rl, oo, ol, st = _arrays(b)
    L.emu_lz4_decompress_batch(C.c_int(variant), E._p(sbuf), C.c_uint64(len(b.stream)), E._p(ro), E._p(rl), C.c_uint32(len(b)),
                               E._p(area), C.c_uint64(b.out_bytes), E._p(oo), E._p(ol), E._p(st))
    return Result(b, area, ol, st)


STAT_NAMES = ("records", "par", "blocks", "slices", "fallback")


def emu_par(b, variant=0, **knobs):
    """min_blocks=None: the emulated gpumt_lz4_decompress_batch_par itself, at its defaults (no stats)"""
    L = E.lib()
    k = dict(KNOBS, **knobs)
    sbuf, area, ro, rl, oo, ol, st = _arrays(b)
    rp, stats = np.full(len(b), 0xA5A5A5A5, np.uint32), np.full(5, 0xA5A5A5A5, np.uint32)
    if k["min_blocks"] is None:
        assert L.gpumt_lz4_decompress_batch_par(C.c_void_p(1), E._p(sbuf), C.c_size_t(len(b.stream)), E._p(ro), E._p(rl),
                                                C.c_size_t(len(b)), E._p(area), C.c_size_t(b.out_bytes), E._p(oo), E._p(ol),
                                                E._p(st), E._p(rp), C.c_int(0)) == 0
        return Result(b, area, ol, st, rp, None)
    L.emu_lz4_decompress_batch_par(C.c_int(variant), E._p(sbuf), C.c_uint64(len(b.stream)), E._p(ro), E._p(rl),
                                   C.c_uint32(len(b)), E._p(area), C.c_uint64(b.out_bytes), E._p(oo), E._p(ol), E._p(st),
                                   E._p(rp), C.c_uint32(k["min_blocks"]), C.c_uint32(k["slice_blocks"]), C.c_int(k["rec_par"]),
                                   C.c_int(k["seg"]), C.c_uint32(k["seg_bytes"]), C.c_uint32(k["cap_mb"]), E._p(stats))
    d = dict(zip(STAT_NAMES, map(int, stats)))
    d["route"] = "seg" if k["seg"] else "par"
    return Result(b, area, ol, st, rp, d)


@contextlib.contextmanager
def captured_stderr(lines):
    """what the process writes to file descriptor 2 inside the block (the library's trace lines) -> appended to `lines`"""
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            lines += f.read().decode(errors="replace").splitlines()


def trace_stats(lines):
    """the `[gpumt lz4 rec] records N par P blocks B slices S fallback F route R` lines -> list of dicts"""
    out = []
    for line in lines:
        if line.startswith("[gpumt lz4 rec]"):
            w = line.split()
            d = {w[i]: int(w[i + 1]) for i in range(3, 13, 2)}
            assert w[13] == "route" and w[14] in ("seg", "par"), line
            d["route"] = w[14]
            out.append(d)
    return out


class Device:
    """the two calls through an Engine that was opened with GPUMT_TRACE=1"""
    VARIANT = dict(min_blocks="lz4_rec_min_blocks", slice_blocks="lz4_rec_slice_blocks", rec_par="lz4_rec_par",
                   seg="lz4_rec_seg", seg_bytes="lz4_seg_bytes", cap_mb="lz4_rec_cap_mb")

    def __init__(self, eng):
        self.eng = eng

    def _run(self, b, par):
        e = self.eng
        sbuf, area, ro, rl, oo, ol, st = _arrays(b)
        n = len(b)
        d_s, d_ro, d_rl, d_oo = e.upload(sbuf, slack=0), e.upload(ro), e.upload(rl), e.upload(oo)
        d_ol, d_st, d_out = e.upload(ol), e.upload(st), e.upload(area, slack=0)
        d_rp = e.upload(np.full(n, 0xA5A5A5A5, np.uint32))
        try:
            if par:
                e.lz4_decompress_par(d_s, len(b.stream), d_ro, d_rl, n, d_out, b.out_bytes, d_oo, d_ol, d_st, d_rp)
            else:
                e.lz4_decompress(d_s, len(b.stream), d_ro, d_rl, n, d_out, b.out_bytes, d_oo, d_ol, d_st)
            e.sync()
            return Result(b, e.download(d_out, len(area)), e.download(d_ol, n * 4, np.uint32),
                          e.download(d_st, n * 4, np.uint32), e.download(d_rp, n * 4, np.uint32) if par else None)
        finally:
            for d in (d_s, d_ro, d_rl, d_oo, d_ol, d_st, d_out, d_rp):
                d.free()

    def serial(self, b, variant=0):
        prev = self.eng.set_variant("lz4_dec", variant)
        try:
            return self._run(b, False)
        finally:
            self.eng.set_variant("lz4_dec", prev)

    def par(self, b, variant=0, **knobs):
        k = dict(KNOBS, **knobs)
        if k["min_blocks"] is None:
            del k["min_blocks"]
        prev = {name: self.eng.set_variant(self.VARIANT[name], v) for name, v in k.items()}
        assert -1 not in prev.values(), prev
        prev_dec = self.eng.set_variant("lz4_dec", variant)
        lines = []
        try:
            with captured_stderr(lines):
                r = self._run(b, True)
        finally:
            self.eng.set_variant("lz4_dec", prev_dec)
            for name, v in prev.items():
                self.eng.set_variant(self.VARIANT[name], v)
        stats = trace_stats(lines)
        assert len(stats) == 1, lines
        r.stats = stats[0]
        return r


def check(b, serial, par, **knobs):
    """both calls on the same batch: status and d_out_len are the serial call's, so are the bytes of every record that
    decoded, and nothing outside the records' ranges is written -> (serial result, par result)"""
    ref, got = serial(b), par(b, **knobs)
    assert list(got.status) == list(ref.status), (list(got.status), list(ref.status))
    assert list(got.out_len) == list(ref.out_len)
    assert ref.gaps_intact() and got.gaps_intact()
    for i in range(len(b)):
        if int(ref.status[i]) == 0:
            assert got.bytes_of(i) == ref.bytes_of(i), i
    return ref, got


# ---- records ----------------------------------------------------------------------------------------------------------------
def nblocks(fr):
    return len(LB.walk(fr)["blocks"])


def block_spans(fr):
    """-> [(offset of the block body in the frame, its size)]"""
    info, out = LB.walk(fr), []
    at = 7 + (8 if fr[4] & 8 else 0) + (4 if fr[4] & 1 else 0)
    for _, body, _ in info["blocks"]:
        out.append((at + 4, len(body)))
        at += 4 + len(body) + (4 if info["bchk"] else 0)
    return out


@functools.lru_cache(maxsize=None)
def text():
    return cases.text(70000, 21)


@functools.lru_cache(maxsize=None)
def hand_specs():
    """name -> (blocks, frame keywords).  Every block of the eligible ones is small: a block needs a declared block
    maximum, not content"""
    t = text()
    h = {}
    # three 100-byte blocks; block 2 has a match whose source starts in block 0 and runs through into block 1
    h["reach_through"] = ([("seq", [(t[:100], 0, 0)]), ("seq", [(t[200:240], 90, 48), (TAIL, 0, 0)]),
                           ("seq", [(t[300:310], 10 + 100 + 50, 78), (TAIL, 0, 0)])], {})
    # off < ml, the source starts 7 bytes before the block
    h["overlap_straddle"] = ([("stored", t[:300]), ("seq", [(b"ab", 2 + 7, 40), (b"", 3, 30), (TAIL, 0, 0)])], {})
    # 20 bytes from before the block, copied on three times inside it
    h["copied_thrice"] = ([("stored", t[:500]), ("seq", [(b"xy", 2 + 30, 20), (b"", 20, 20), (b"q", 21, 20), (b"", 41, 20),
                                                         (TAIL, 0, 0)])], {})
    h["stored_and_empty_stored"] = ([("seq", [(t[:900], 100, 400), (TAIL, 0, 0)]), ("stored", t[2000:4000]), ("stored", b""),
                                     ("seq", [(b"xyz", 2000 + 30, 64), (b"", 80, 64), (TAIL, 0, 0)])], {})
    h["full_64k_then_65535"] = ([("stored", t[:65536]), ("seq", [(b"", 65535, 40), (b"abc", 65535, 300), (TAIL, 0, 0)])], {})
    h["bcheck_dictid"] = (h["reach_through"][0], dict(bcheck=True, dict_id=77))
    h["five_blocks"] = ([("stored", t[:50]), ("seq", [(t[60:70], 40, 30), (TAIL, 0, 0)]), ("stored", b""), ("stored", t[:33]),
                         ("seq", [(b"Z", 100, 90), (TAIL, 0, 0)])], {})
    # errors the run decoders find: an offset larger than the bytes decoded so far, an end-of-block rule in a middle block
    h["err_offset_beyond"] = ([("seq", [(t[:100], 0, 0)]), ("seq", [(t[200:240], 90, 48), (TAIL, 0, 0)]),
                               ("seq", [(b"abc", 3 + 200 + 1, 40), (TAIL, 0, 0)])], {})
    h["err_end_of_block_rule"] = ([("stored", t[:100]), ("seq", [(t[:20], 10, 40), (b"abc", 0, 0)]), ("stored", t[:60])], {})
    # not eligible
    h["one_block"] = ([("seq", [(t[:50], 20, 40), (TAIL, 0, 0)])], {})
    h["independent"] = ([("stored", t[:80]), ("seq", [(t[:50], 20, 40), (TAIL, 0, 0)])], dict(indep=True))
    h["no_content_size"] = (h["reach_through"][0], dict(csize=False))
    return h


HAND_ELIGIBLE = ("reach_through", "overlap_straddle", "copied_thrice", "stored_and_empty_stored", "full_64k_then_65535",
                 "bcheck_dictid", "five_blocks")
HAND_ERRORS = ("err_offset_beyond", "err_end_of_block_rule")
HAND_OTHER = ("one_block", "independent", "no_content_size")
EDGE = "reach_through"


@functools.lru_cache(maxsize=None)
def hand(name):
    """-> (frame, content or None when the blocks do not decode, number of blocks)"""
    blocks, kw = hand_specs()[name]
    try:
        want = S.content(blocks, kw.get("indep", False))
    except ValueError:
        want = None
    if name == "err_end_of_block_rule":
        want = None
    return S.frame(blocks, **kw), want, len(blocks)


def cap_of(name):
    """what the caller passes in d_out_len: the content size, or a capacity for the frame that states none"""
    fr, want, _ = hand(name)
    if not fr[4] & 0x08:
        return len(want) + 100
    return struct.unpack_from("<Q", fr, 6)[0]


def bad_magic_record():
    r = bytearray(S.record(hand(EDGE)[0]))
    r[0] ^= 1
    return bytes(r)


def bad_header_checksum_record():
    fr = bytearray(hand(EDGE)[0])
    fr[14] ^= 0x40                     # the HC byte behind FLG, BD and the 8-byte content size
    return S.record(bytes(fr))


def mixed_batch():
    """the hand-built records, eligible ones, failing ones and ineligible ones in turn -> (Batch, names)"""
    order = ["reach_through", "one_block", "overlap_straddle", "independent", "copied_thrice", "err_offset_beyond",
             "no_content_size", "stored_and_empty_stored", "bad_magic", "full_64k_then_65535", "err_end_of_block_rule",
             "bad_header_checksum", "bcheck_dictid", "five_blocks"]
    recs = []
    for n in order:
        if n == "bad_magic":
            recs.append((bad_magic_record(), cap_of(EDGE)))
        elif n == "bad_header_checksum":
            recs.append((bad_header_checksum_record(), cap_of(EDGE)))
        else:
            recs.append((S.record(hand(n)[0]), cap_of(n)))
    return Batch(recs), order


def edge_frames():
    """name -> (frame, out_len on entry): what is wrong around the blocks of the 3-block frame"""
    blocks, _ = hand_specs()[EDGE]
    fr, want, _ = hand(EDGE)
    n = len(want)
    c = {}
    c["content_size_plus_1"] = (S.frame(blocks, content_size=n + 1), n + 1)
    c["content_size_minus_1"] = (S.frame(blocks, content_size=n - 1), n - 1)
    c["content_checksum_flipped"] = (fr[:-2] + bytes([fr[-2] ^ 0x10]) + fr[-1:], n)
    bc = bytearray(S.frame(blocks, bcheck=True))
    off, size = block_spans(bytes(bc))[1]
    bc[off + size + 1] ^= 0x04                            # a byte of the second block's checksum
    c["block_checksum_flipped"] = (bytes(bc), n)
    c["no_end_mark"] = (S.frame(blocks, endmark=False), n)
    c["trailing_byte"] = (fr + b"\0", n)
    at = sum(block_spans(fr)[-1])
    c["last_block_truncated"] = (fr[:at - 1] + fr[at:], n)
    return c


def edge_records():
    c = {k: (S.record(fr), n) for k, (fr, n) in edge_frames().items()}
    fr, want, _ = hand(EDGE)
    r = bytearray(S.record(fr))
    r[8:12] = struct.pack("<I", len(fr) + 1)
    c["record_csize_plus_1"] = (bytes(r), len(want))
    c["out_len_differs"] = (S.record(fr), len(want) + 5)
    return c


def n_block_record(n, seed=0):
    """n blocks: stored ones of 40 bytes and a last block that reaches back over them, at most 60 000 bytes"""
    t = text()
    blocks = [("stored", t[seed + 40 * k:seed + 40 * k + 40]) for k in range(n - 1)]
    blocks.append(("seq", [(b"ab", 2 + 40 * min(n - 1, 1500), 30), (TAIL, 0, 0)]))
    fr = S.frame(blocks)
    return S.record(fr), len(S.content(blocks)), S.content(blocks)


def slice_batch(lead=0):
    """six 3-block records"""
    recs = [n_block_record(3, seed=100 * k) for k in range(6)]
    return Batch([(r, c) for r, c, _ in recs], lead=lead), [w for _, _, w in recs]


def many_blocks_batch(nrec=70, nblk=1000):
    """records of one stored byte and nblk - 1 empty stored blocks each: 70 000 blocks, whose table is more than 1 MiB"""
    blocks = [("stored", b"x")] + [("stored", b"")] * (nblk - 1)
    fr = S.frame(blocks)
    return Batch([(S.record(fr), 1)] * nrec)


@functools.lru_cache(maxsize=None)
def seg_one_block():
    """one block of 3000 bytes with matches all along"""
    b = G.Bld(31)
    b.seq(30, 10, 40)
    b.land_on(3000 - 12)
    blocks = [b.end()]
    want = S.content(blocks)
    assert len(want) == 3000
    return S.frame(blocks), want


@functools.lru_cache(maxsize=None)
def seg_big_blocks():
    """BD = 4 MiB, two linked blocks of about 200 KiB of text"""
    import lz4_seg_api as GA
    blocks = GA._blocks([200000, 200000], True, 140)
    return S.frame(blocks, bd=7), S.content(blocks)


def rec_manifest():
    with open(REC_MANIFEST) as f:
        return json.load(f)


def manifest_frames():
    """name -> frame of everything tests/golden/gen_golden_lz4_rec.py records liblz4's verdict for"""
    out = {n: hand(n)[0] for n in HAND_ELIGIBLE + HAND_ERRORS + HAND_OTHER}
    out.update({"edge_" + k: fr for k, (fr, _) in edge_frames().items()})
    out["seg_one_block"] = seg_one_block()[0]
    out["seg_big_blocks"] = seg_big_blocks()[0]
    return out


def dump_cases(path):
    """the inputs of tools/lz4_rec_san.sh: the mixed batch (whole, in slices of 2 blocks, on the seg route with segments of
    256 bytes), the edge cases and the slice batch -> number of cases"""
    out = []

    def add(b, min_blocks=2, slice_blocks=4096, seg=0, seg_bytes=65536):
        out.append(struct.pack("<7I", len(b.stream), len(b), b.out_bytes, min_blocks, slice_blocks, seg, seg_bytes) + b.stream +
                   b.rec_off.tobytes() + b.rec_len.tobytes() + b.out_off.tobytes() + b.cap.tobytes())
    add(mixed_batch()[0])
    add(mixed_batch()[0], slice_blocks=2)
    add(mixed_batch()[0], seg=1, seg_bytes=256)
    add(Batch(list(edge_records().values())))
    add(Batch(list(edge_records().values())), seg=1, seg_bytes=256)
    add(slice_batch(lead=600)[0], slice_blocks=4)
    add(Batch([(S.record(seg_one_block()[0]), 3000)]), seg=1, seg_bytes=256)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(out))
    return len(out)
