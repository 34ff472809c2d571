"""Sequence-level zstd frame builder (TEST CODE ONLY).

A frame is a list of blocks, each one of
  ("raw", data)                     a Raw_Block, may be empty;
  ("rle", byte, n)                  an RLE_Block of n bytes;
  ("comp", literals, sequences)     a Compressed_Block (RFC 8878 3.1.1.3), see lit() and seq();
  ("bytes", body, type)             any block bytes, for malformed input the other forms cannot express.
The builder writes the Huffman and FSE bitstreams itself (plain Python, big integers), the frame header with every
choice, and the 12-byte zstd-mt record.  `content()` decodes the description the plain sequential way with its own
repeat-offset history: that is the expected output.  It shares no code with the kernels, the oracle or
helpers.zstd_rle_mode_frame; what validates it is libzstd (tests/golden/gen_golden_zstd_synth.py).
"""
import ctypes as C
import hashlib
import heapq
import os
import random
import struct

import xxhash

MAGIC = bytes([0x28, 0xB5, 0x2F, 0xFD])
SKIP_MAGIC = 0x184D2A50
ST_OK, ST_BAD_FRAME, ST_BAD_BLOCK, ST_SIZE_MISMATCH, ST_BAD_CHECKSUM = 0, 2, 3, 4, 5

LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(bits, first):
    out = [first]
    for b in bits[:-1]:
        out.append(out[-1] + (1 << b))
    return out


LL_BASE, ML_BASE = _bases(LL_BITS, 0), _bases(ML_BITS, 3)
assert LL_BASE[25] == 64 and LL_BASE[35] == 65536 and ML_BASE[43] == 131 and ML_BASE[52] == 65539
# predefined distributions, RFC 8878 3.1.1.3.2.2
PRE_LL = ([4, 3] + [2] * 11 + [1, 1, 1] + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4, 6)
PRE_OF = ([1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5, 5)
PRE_ML = ([1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7, 6)
MAX_AL = (9, 8, 9)          # LL, OF, ML
MAX_SYM = (35, 31, 52)


def ll_code(ll):
    return max(i for i in range(36) if LL_BASE[i] <= ll)


def ml_code(ml):
    return max(i for i in range(53) if ML_BASE[i] <= ml)


def of_code(ofv):
    return ofv.bit_length() - 1


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


# ---- bit writers ------------------------------------------------------------------------------------------------------
def backward(items, marker=True):
    """items = (value, nbits) in the order a decoder reads them -> the bytes of a stream read from its end: the first
    item sits right under the padding marker (the highest set bit of the last byte)"""
    s = "".join(format(v, "0%db" % nb) for v, nb in items if nb)
    assert all(0 <= v < (1 << nb) for v, nb in items if nb) and all(v == 0 for v, nb in items if not nb)
    acc = int(("1" if marker else "0") + s, 2)
    return acc.to_bytes((len(s) + 1 + 7) // 8, "little")


class Forward:
    """a stream read from its first byte, least significant bit first (FSE table descriptions)"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb)
        self.acc |= v << self.n
        self.n += nb

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- FSE --------------------------------------------------------------------------------------------------------------
def fse_table(norm, al):
    """decode table by the RFC's spread (4.1.1): list of (symbol, nbits, base)"""
    size = 1 << al
    assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
    sym, high = [None] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [1 if c == -1 else c for c in norm]
    out = []
    for s in sym:
        x = nxt[s]
        nxt[s] += 1
        nb = al - (x.bit_length() - 1)
        out.append((s, nb, (x << nb) - size))
    return out


def fse_describe(norm, al, fw=None):
    """the table description (4.1.1): accuracy log, then every probability with its variable width, zero runs through the
    2-bit repeat flags; trailing zero probabilities are not written"""
    fw = fw or Forward()
    fw.put(al - 5, 4)
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    s, prev0, n = 0, False, len(norm)
    while n and norm[n - 1] == 0:
        n -= 1
    while s < n and remaining > 1:
        if prev0:
            start = s
            while norm[s] == 0:
                s += 1
            while s >= start + 3:
                fw.put(3, 2)
                start += 3
            fw.put(s - start, 2)
        c = norm[s]
        s += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        c += 1
        if c >= threshold:
            c += mx
        fw.put(c, nbits - (1 if c < mx else 0))
        prev0 = c == 1
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    assert remaining == 1 and s == n
    return fw


def fse_states(table, syms):
    """states of one FSE stream, chosen backwards: the last symbol takes its first cell, every earlier one the cell of
    its symbol whose [base, base + 2^nb) holds the following state -> (list of states, list of (bits, nb) read after
    symbol i to reach state i + 1)"""
    cells = {}
    for i, (s, nb, base) in enumerate(table):
        cells.setdefault(s, []).append(i)
    st = [None] * len(syms)
    upd = [None] * (len(syms) - 1)
    st[-1] = max(cells[syms[-1]], key=lambda i: (table[i][1], -i))
    for i in range(len(syms) - 2, -1, -1):
        nx = st[i + 1]
        for c in cells[syms[i]]:
            _, nb, base = table[c]
            if base <= nx < base + (1 << nb):
                st[i], upd[i] = c, (nx - base, nb)
                break
        else:
            raise AssertionError("no cell of symbol %d reaches state %d" % (syms[i], nx))
    return st, upd


def normalize(hist, al, minus1=False):
    """counts -> normalised counts that sum to 2^al, every present symbol at least 1 (or -1: "less than one", when
    minus1 and it would get 1)"""
    size, total = 1 << al, sum(hist)
    assert sum(1 for h in hist if h) <= size
    norm = [max(1, h * size // total) if h else 0 for h in hist]
    while sum(norm) != size:
        d = size - sum(norm)
        i = max(range(len(norm)), key=lambda k: norm[k])
        norm[i] += d if d > 0 else max(d, 1 - norm[i])
    if minus1:
        norm = [-1 if c == 1 else c for c in norm]
    return norm


# ---- Huffman ----------------------------------------------------------------------------------------------------------
def huf_weights(data, maxbits=11, exact_max=False):
    """weights (0 = absent) of the bytes in `data` for codes of at most `maxbits` bits; exact_max makes the longest code
    exactly maxbits long (needs enough symbols)"""
    hist = [0] * 256
    for b in data:
        hist[b] += 1
    present = [s for s in range(256) if hist[s]]
    assert len(present) >= 2
    heap = [(hist[s], s, (s,)) for s in present]
    heapq.heapify(heap)
    ln = dict.fromkeys(present, 0)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            ln[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    if exact_max:                       # a chain: lengths 1, 2, ..., then the rest share what is left
        order = sorted(present, key=lambda s: (-hist[s], s))
        assert len(order) > maxbits
        for i, s in enumerate(order):
            ln[s] = min(i + 1, maxbits)
    full = 1 << maxbits
    for s in present:
        ln[s] = min(ln[s], maxbits)
    kraft = lambda: sum(full >> ln[s] for s in present)  # noqa: E731
    while kraft() > full:               # too many short codes: lengthen the longest code that can grow
        s = max((s for s in present if ln[s] < maxbits), key=lambda s: (ln[s], -hist[s]))
        ln[s] += 1
    while kraft() < full:               # room left: shorten the longest code that fits
        d = full - kraft()
        s = max((s for s in present if ln[s] > 1 and (full >> ln[s]) <= d), key=lambda s: (ln[s], hist[s]))
        ln[s] -= 1
    top = max(ln.values())
    return [top + 1 - ln[s] if hist[s] else 0 for s in range(max(present) + 1)]


def huf_codes(weights):
    """weights of symbols 0..n-1, the last one included -> {symbol: (code, length)}: cells are handed out by rising
    weight, symbols of one weight in rising order (4.2.1)"""
    total = sum(1 << (w - 1) for w in weights if w)
    maxbits = total.bit_length() - 1
    assert total == 1 << maxbits, "weights do not fill a power of two"
    codes, pos = {}, 0
    for w in range(1, maxbits + 2):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (pos >> (w - 1), maxbits + 1 - w)
                pos += 1 << (w - 1)
    return codes


def huf_tree_desc(weights, fse=False, al=6):
    """Huffman_Tree_Description of `weights` (the last symbol's weight is implied, not written)"""
    w = weights[:-1]
    assert weights[-1] != 0
    if not fse:
        assert 1 <= len(w) <= 128
        w = w + [0] * (len(w) & 1)
        return bytes([127 + len(weights) - 1]) + bytes(w[i] << 4 | w[i + 1] for i in range(0, len(w), 2))
    hist = [0] * (max(w) + 1)
    for x in w:
        hist[x] += 1
    norm = normalize(hist, al)
    table = fse_table(norm, al)
    # two states take turns (4.2.1.2): state 1 the even weights, state 2 the odd ones; each state's last symbol sits in
    # a cell that needs bits, so the decoder finds the stream exhausted when it updates past it
    assert len(w) >= 2
    s1, u1 = fse_states(table, w[0::2])
    s2, u2 = fse_states(table, w[1::2])
    assert table[s1[-1]][1] > 0 and table[s2[-1]][1] > 0
    items = [(s1[0], al), (s2[0], al)]
    for i in range(len(w)):
        u = (u1 if i % 2 == 0 else u2)
        if i // 2 < len(u):
            items.append(u[i // 2])
    body = fse_describe(norm, al).bytes() + backward(items)
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def huf_stream(data, codes):
    return backward([codes[b] for b in data])


# ---- specs ------------------------------------------------------------------------------------------------------------
def lit(kind, data=b"", sf=None, streams=None, weights=None, maxbits=11, fse=False, exact_max=False, **over):
    """literals spec.  kind: "raw" | "rle" | "huf" | "treeless".  sf = Size_Format (None: the smallest that fits);
    streams 1 or 4; weights passed in (list over symbols 0..last, last included) or derived from the data with codes of
    at most maxbits; fse = FSE-compressed weights.  over: regen / csz (header fields), tree (description bytes),
    jump (the three jump-table sizes), streams_bytes (list of stream bytes) replace what the builder would write."""
    if kind == "rle":
        assert len(set(data)) <= 1
    return dict(kind=kind, data=bytes(data), sf=sf, streams=streams, weights=weights, maxbits=maxbits, fse=fse,
                exact_max=exact_max, over=over)


def seq(seqs, ll="pre", of="pre", ml="pre", form=None, **over):
    """sequences spec: seqs = [(ll, ml, offset_value)]; a mode is "pre" | "rle" | "rep" | ("fse", al) (counts fitted to
    the block's codes) | ("fse", al, norm) | ("fse", al, norm_or_None, "minus1").  form = bytes of Number_of_Sequences
    (None: the shortest).  over: nseq (the number written), bits (function: bitstream bytes -> bytes), desc (function
    (table index, description bytes) -> bytes)."""
    return dict(seqs=list(seqs), modes=(ll, of, ml), form=form, over=over)


class _State:
    """what later blocks of a frame may refer to: the last Huffman codes and the last three FSE tables"""

    def __init__(self):
        self.huf = None
        self.tab = [None, None, None]


def _lit_bytes(L, st):
    kind, data, over = L["kind"], L["data"], L["over"]
    regen = over.get("regen", len(data))
    if kind in ("raw", "rle"):
        sf = L["sf"] if L["sf"] is not None else (0 if regen < 32 else 1 if regen < 4096 else 3)
        hl = (1, 2, 1, 3)[sf]
        t = 0 if kind == "raw" else 1
        v = t | sf << 2 | regen << (3 if hl == 1 else 4)
        assert regen < (1 << (5 if hl == 1 else 12 if hl == 2 else 20))
        return v.to_bytes(hl, "little") + (data if kind == "raw" else data[:1])
    tree = b""
    if kind == "huf":
        w = L["weights"] if L["weights"] is not None else huf_weights(data, L["maxbits"], L["exact_max"])
        tree = over["tree"] if "tree" in over else huf_tree_desc(w, L["fse"])
        try:
            st.huf = huf_codes(w)
        except AssertionError:
            if "streams_bytes" not in over:
                raise
    codes = st.huf
    nstreams = L["streams"] or (1 if regen < 1024 and L["sf"] in (None, 0) else 4)
    if "streams_bytes" in over:
        parts = over["streams_bytes"]
    elif nstreams == 1:
        parts = [huf_stream(data, codes)]
    else:
        q = (len(data) + 3) // 4
        parts = [huf_stream(data[i * q:(i + 1) * q], codes) for i in range(4)]
    body = tree
    if nstreams == 4:
        jump = over.get("jump", tuple(len(p) for p in parts[:3]))
        body += struct.pack("<HHH", *jump)
    body += b"".join(parts)
    csz = over.get("csz", len(body))
    if L["sf"] is not None:
        sf = L["sf"]
    elif nstreams == 1:
        sf = 0
    else:
        sf = 1 if max(regen, csz) < 1024 else 2 if max(regen, csz) < 16384 else 3
    assert (sf == 0) == (nstreams == 1)
    bits, hl = (10, 10, 14, 18)[sf], (3, 3, 4, 5)[sf]
    assert regen < (1 << bits) and csz < (1 << bits), (regen, csz, sf)
    v = (2 if kind == "huf" else 3) | sf << 2 | regen << 4 | csz << (4 + bits)
    return v.to_bytes(hl, "little") + body


def _table_for(mode, t, codes, st):
    """-> (mode number, description bytes, (table, al))"""
    pre = (PRE_LL, PRE_OF, PRE_ML)[t]
    if mode == "pre":
        return 0, b"", (fse_table(*pre), pre[1])
    if mode == "rle":
        assert len(set(codes)) == 1
        return 1, bytes([codes[0]]), ([(codes[0], 0, 0)], 0)
    if mode == "rep":
        return 3, b"", st.tab[t]
    al = mode[1]
    norm = mode[2] if len(mode) > 2 and mode[2] is not None else None
    if norm is None:
        hist = [0] * (max(codes) + 1)
        for c in codes:
            hist[c] += 1
        norm = normalize(hist, al, minus1=len(mode) > 3)
    return 2, fse_describe(norm, al).bytes(), (fse_table(norm, al), al)


def _seq_bytes(S, st):
    seqs, over = S["seqs"], S["over"]
    n = over.get("nseq", len(seqs))
    form = S["form"] or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        head = bytes([n])
    elif form == 2:
        assert n < 0x7F00
        head = bytes([128 + (n >> 8), n & 255])
    else:
        assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
        head = b"\xff" + struct.pack("<H", n - 0x7F00)
    if not seqs:
        return head + over.get("tail", b"")
    cl = [ll_code(a) for a, _, _ in seqs]
    co = [of_code(o) for _, _, o in seqs]
    cm = [ml_code(m) for _, m, _ in seqs]
    out, tabs, modes = bytearray(), [], 0
    for t, codes in enumerate((cl, co, cm)):
        m, desc, tab = _table_for(S["modes"][t], t, codes, st)
        if "desc" in over:
            desc = over["desc"](t, desc)
        modes |= m << (6 - 2 * t)
        out += desc
        tabs.append(tab)
        if tab is not None:
            st.tab[t] = tab
    (tl, al_l), (to, al_o), (tm, al_m) = tabs
    sl, ul = fse_states(tl, cl)
    so, uo = fse_states(to, co)
    sm, um = fse_states(tm, cm)
    items = [(sl[0], al_l), (so[0], al_o), (sm[0], al_m)]
    for i, (a, m, o) in enumerate(seqs):
        items += [(o - (1 << co[i]), co[i]), (m - ML_BASE[cm[i]], ML_BITS[cm[i]]), (a - LL_BASE[cl[i]], LL_BITS[cl[i]])]
        if i + 1 < len(seqs):
            items += [ul[i], um[i], uo[i]]
    bits = backward(items)
    if "bits" in over:
        bits = over["bits"](bits)
    return head + bytes([over.get("modes", modes)]) + bytes(out) + bits


def block_body(b, st):
    """(type, body bytes, size field) of one block"""
    if b[0] == "raw":
        return 0, b[1], len(b[1])
    if b[0] == "rle":
        return 1, bytes([b[1]]), b[2]
    if b[0] == "bytes":
        return b[2], b[1], (b[3] if len(b) > 3 else len(b[1]))
    body = _lit_bytes(b[1], st) + _seq_bytes(b[2], st)
    return 2, body, len(body)


# ---- content ----------------------------------------------------------------------------------------------------------
def decode_block(L, S, out: bytearray, rep, block_max=131072, trace=None):
    """append what a compressed block decodes to; rep = the three repeat offsets (updated in place).  Raises ValueError
    on what RFC 8878 forbids"""
    data, start, lp = L["data"], len(out), 0
    if L["kind"] == "rle":
        data = data[:1] * L["over"].get("regen", len(data))
    for a, m, o in S["seqs"]:
        if lp + a > len(data):
            raise ValueError("sequences need more literals than the block has")
        out += data[lp:lp + a]
        lp += a
        if o > 3:
            off = o - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = o + (1 if a == 0 else 0)           # 3.1.1.5: a literals length of 0 shifts the repeat code by one
            if idx == 1:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 4 else rep[idx - 1]
                if off == 0:
                    raise ValueError("repeat offset 1 minus 1 byte is 0")
                if idx == 2:
                    rep[:] = [off, rep[0], rep[2]]
                else:
                    rep[:] = [off, rep[0], rep[1]]
        if off > len(out):
            raise ValueError("offset %d reaches before the start (%d bytes)" % (off, len(out)))
        if trace is not None:
            trace.append((len(out), off))
        s = len(out) - off
        if off >= m:
            out += out[s:s + m]
        else:
            for j in range(m):
                out.append(out[s + j])
    out += data[lp:]
    if len(out) - start > block_max:
        raise ValueError("block decodes to more than Block_Maximum_Size")


def content(blocks, block_max=131072, trace=None):
    """the decoded content of a frame, sequentially.  Raises ValueError where the RFC forbids the description; a "bytes"
    block has no description: ValueError too"""
    out, rep = bytearray(), [1, 4, 8]
    for b in blocks:
        if b[0] == "raw":
            if len(b[1]) > block_max:
                raise ValueError("raw block above Block_Maximum_Size")
            out += b[1]
        elif b[0] == "rle":
            if b[2] > block_max:
                raise ValueError("RLE block above Block_Maximum_Size")
            out += bytes([b[1]]) * b[2]
        elif b[0] == "comp":
            decode_block(b[1], b[2], out, rep, block_max, trace)
        else:
            raise ValueError("block given as bytes")
    return bytes(out)


# ---- frames -----------------------------------------------------------------------------------------------------------
def nominal_size(blocks):
    """what a frame states as its content size when its description cannot be decoded: literals plus match lengths"""
    n = 0
    for b in blocks:
        if b[0] == "comp":
            n += b[1]["over"].get("regen", len(b[1]["data"])) + sum(m for _, m, _ in b[2]["seqs"])
        elif b[0] != "bytes":
            n += len(b[1]) if b[0] == "raw" else b[2]
    return n


def frame(blocks, fcs=None, single=None, window=None, did=None, did_width=None, reserved=0, unused=0, checksum=None,
          content_size=None, last=True):
    """zstd frame of `blocks`.  fcs = bytes of the Frame_Content_Size field (0, 1, 2, 4, 8; None: the smallest that
    holds it); single = Single_Segment (None: set when the 1-byte field is used, which needs it); window = (exponent,
    mantissa) of the Window_Descriptor; did_width 0/1/2/4 with id `did`; checksum: None = none, True = the right one,
    an int = that value; content_size overrides the field; last=False leaves the Last_Block bit of the last block off"""
    try:
        data = content(blocks)
    except ValueError:
        data = None
    n = content_size if content_size is not None else len(data) if data is not None else nominal_size(blocks)
    if fcs is None:
        fcs = 2 if 256 <= n < 65536 + 256 else 4
    if single is None:
        single = fcs == 1
    assert fcs in (0, 1, 2, 4, 8) and (fcs != 1 or single) and (fcs != 0 or not single)
    did_width = did_width if did_width is not None else 0
    fhd = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs] << 6 | (1 if single else 0) << 5 | unused << 4 | reserved << 3 | \
        (4 if checksum is not None else 0) | {0: 0, 1: 1, 2: 2, 4: 3}[did_width]
    out = bytearray(MAGIC + bytes([fhd]))
    if not single:
        e, m = window if window is not None else (7, 0)
        out.append(e << 3 | m)
    out += (did or 0).to_bytes(did_width, "little")
    if fcs:
        out += (n - 256 if fcs == 2 else n).to_bytes(fcs, "little")
    st = _State()
    for i, b in enumerate(blocks):
        typ, body, size = block_body(b, st)
        assert size < 1 << 21
        out += ((1 if last and i == len(blocks) - 1 else 0) | typ << 1 | size << 3).to_bytes(3, "little") + body
    if checksum is not None:
        v = checksum if checksum is not True else xxhash.xxh64(data or b"", seed=0).intdigest() & 0xFFFFFFFF
        out += struct.pack("<I", v)
    return bytes(out)


def record(fr: bytes) -> bytes:
    """zstd-mt skippable record: magic, 4, frame size, frame"""
    return struct.pack("<III", SKIP_MAGIC, 4, len(fr)) + fr


def has_fcs(fr: bytes) -> bool:
    return (fr[4] >> 6) != 0 or ((fr[4] >> 5) & 1) != 0


# ---- libzstd's verdict (the image's libzstd 1.4.9) ---------------------------------------------------------------------
LIBZSTD = "/opt/conda/lib/libzstd.so.1"
_zs = None


def libzstd_decompress(fr: bytes, cap: int = 5 << 20):
    """ZSTD_decompress over the frame -> (accepted, content bytes or None); None if libzstd is not on this machine"""
    global _zs
    if not os.path.exists(LIBZSTD):
        return None
    if _zs is None:
        _zs = C.CDLL(LIBZSTD)
        _zs.ZSTD_decompress.restype = C.c_size_t
        _zs.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        _zs.ZSTD_isError.restype = C.c_uint
        _zs.ZSTD_isError.argtypes = [C.c_size_t]
        _zs.ZSTD_versionNumber.restype = C.c_uint
    dst = C.create_string_buffer(cap)
    rv = _zs.ZSTD_decompress(dst, cap, fr, len(fr))
    if _zs.ZSTD_isError(rv):
        return False, None
    return True, dst.raw[:rv]


def libzstd_version():
    libzstd_decompress(b"")
    return _zs.ZSTD_versionNumber() if _zs is not None else None


# ---- families ---------------------------------------------------------------------------------------------------------
# Cases where libzstd 1.4.9 accepts and RFC 8878 forbids: name -> the sentence that decides.  Expected verdict: rejected.
_REP0 = ("RFC 8878 3.1.1.5: \"an offset_value of 3 [with literals_length 0] means Repeated_Offset1 - 1_byte\"; 3.1.1.4: "
         "an offset of 0 is not a valid match distance, and 3.1.1.5 as revised (and libzstd from 1.5.5) calls the "
         "resulting 0 corrupted data; libzstd 1.4.9 decodes it as offset 1")
_BMAX = ("RFC 8878 3.1.1.2.3: \"Block_Size is limited by Block_Maximum_Size\"; 3.1.1.2.4: \"Block_Maximum_Size is the smallest of: Window_Size, 128 KB\" and \"A Compressed_Block has "
         "the extra restriction that Block_Size is always strictly less than the decompressed size ... the decompressed "
         "size [is limited] to Block_Maximum_Size\"; libzstd 1.4.9's one-shot decoder holds blocks to 128 KB only")
DIVERGENT = {
    "rep_rep0_minus1_zero": _REP0,
    "rep_rep0_minus1_zero_later": _REP0,
    "sp_rep_rep0_minus1_zero": _REP0,
    "huf_bad_12bit": "RFC 8878 4.2.1: \"Zstandard Huffman-coded streams ... limits its maximum Number_of_Bits to 11\"; "
                     "libzstd 1.4.9 builds its literals table for 12",
    "seq_bad_one_byte_long": "RFC 8878 4.1: \"If the bitstream is not entirely and exactly consumed, hence reaching exactly "
                             "its beginning position with all bits consumed, the decoding process is considered faulty\"; "
                             "libzstd 1.4.9 does not look at what is left of the sequences bitstream",
    "window_1k_block_over": _BMAX,
    "out_block_max_plus1": _BMAX,
    "ml_131074_single": _BMAX,
    "seq_bad_modes_reserved": "RFC 8878 3.1.1.3.2.1 (Symbol_Compression_Modes): \"The last field, Reserved, must be "
                              "all zeroes\"; libzstd 1.4.9 does not look at the two bits",
    "hdr_single_block_above_window": _BMAX,
    "window_1k_raw_over": _BMAX,
}


class _Fam:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.cases = {}
        self.why = {}
        self.bad = []

    def text(self, n, alphabet=b"abcdefghijklmnopqrstuvwxyz ,.ETAOIN"):
        return bytes(self.rng.choice(alphabet) for _ in range(n))

    def skew(self, n, nsym=40, base=32):
        """bytes with a geometric-like distribution over nsym symbols: Huffman codes of many lengths"""
        w = [max(1, int(4000 * 0.8 ** i)) for i in range(nsym)]
        return bytes(self.rng.choices(range(base, base + nsym), w, k=n))

    def add(self, name, blocks, status=ST_OK, level=None, **fk):
        """level: for a rejected case, "block" when decoding the blocks themselves must fail, "frame" when the blocks
        decode and the frame around them is what is wrong (header, content size, checksum)"""
        assert name not in self.cases, name
        trace = []
        try:
            data = content(blocks, fk.pop("block_max", 131072), trace)
        except ValueError as e:
            data, self.why[name] = None, str(e)
        # matches (output position, offset) that reach beyond the Window_Size the header states
        e_, m_ = fk.get("window") or (7, 0)
        win = (1 << (10 + e_)) + ((1 << (10 + e_)) >> 3) * m_
        far = [(p, o) for p, o in trace if o > win] if not fk.get("single") and fk.get("fcs") != 1 else []
        if status == ST_OK and data is None:
            self.bad.append("%s: built as valid, and content() refuses it: %s" % (name, self.why[name]))
        if status not in (ST_OK, None) and level is None:
            level = "block"
        self.cases[name] = {"frame": frame(blocks, **fk), "content": data, "status": status, "level": level,
                            "far": far}


def families(seed=1):
    F = _Fam(seed)
    T = F.text
    B = ST_BAD_BLOCK

    def rawlit(seqs, extra=0):
        return lit("raw", T(sum(a for a, _, _ in seqs) + extra))

    def comp(seqs, extra=0, **sk):
        return ("comp", rawlit(seqs, extra), seq(seqs, **sk))

    hist128k = [("rle", 0x5A, 131072)]

    # ---- sequence count forms ----
    F.add("nseq_0", [("comp", lit("raw", T(40)), seq([]))])
    for n in (1, 127, 128):
        F.add("nseq_%d" % n, [comp([(2, 4, 5)] + [(1, 3, 6 + i % 5) for i in range(n - 1)], 3)])
    for n in (0x7EFF, 0x7F00):
        F.add("nseq_0x%X" % n, [comp([(1, 3, 4)] + [(0, 3, 4 + i % 3 * 3) for i in range(n - 1)], 1)])
    F.add("nseq_127_form2", [comp([(2, 4, 5)] + [(1, 3, 6)] * 126, 3, form=2)])
    # more than Z_SEQCAP (24576) and more than block_max / 4 (32768): 3-byte matches behind one literal
    n = 40000
    F.add("nseq_above_seqcap", [comp([(4, 3, 5)] + [(0, 3, 4 + (i % 4)) for i in range(n - 1)], 0)])
    assert 3 * n + 4 <= 131072

    # ---- batches of 64 ----
    for n in (63, 64, 65, 128, 129):
        F.add("batch_%d" % n, [comp([(13, 5, 7)] + [(i % 3, 3 + i % 6, 4 + i % 11) for i in range(1, n)], 2)])
    # 64 sequences that each carry the most extra bits the codes allow inside 128 KiB: LL code 25+ / ML code 43+ /
    # offset code 17 need RLE history; here LL code 24 (4 bits), ML code 42 (5 bits), offset code 16 (16 bits) per
    # sequence plus 6 + 5 + 6 state bits
    pre = [("rle", 0x33, 70000)]
    F.add("batch_64_max_bits", pre + [comp([(48 + 15, 99 + 31, 65536 + 3000 + i) for i in range(64)], 5,
                                           ll=("fse", 6), of=("fse", 5), ml=("fse", 6))])
    F.add("batch_64_big_codes", hist128k + [comp([(64 + i, 131 + i, (1 << 16) + 100 + i) for i in range(64)], 5)])
    # a last sequence that needs no bits at all: codes without extra bits, reached by a 0-bit state update
    F.add("batch_last_no_bits", [("raw", T(5)), comp([(6, 6, 1)] * 70, 0, ll="rle", of="rle", ml="rle")])
    F.add("batch_last_no_extra_bits", [comp([(400, 40, 300), (3, 4, 1)], 0)])

    # ---- copy widths ----
    for v in (0, 1, 7, 8, 9, 64, 65):
        F.add("ll_%d" % v, [comp([(30, 10, 20), (v, 5, 12), (v, 6, 2), (v, 4, 30)], 2)])
        if v >= 3:
            F.add("ml_%d" % v, [comp([(80, v, 75), (2, v, 6), (0, v, 4), (1, v, 2)], 2)])
    F.add("ml_3", [comp([(80, 3, 75), (2, 3, 6), (0, 3, 4)], 2)])
    F.add("long_head_of_batch", [comp([(3000, 5000, 2500)] + [(2, 5, 9)] * 70, 4)])
    F.add("long_mid_batch", [comp([(3, 5, 6)] * 30 + [(2000, 4000, 1000)] + [(2, 5, 9)] * 50, 4)])
    F.add("long_at_64_boundary", [comp([(3, 5, 6)] * 63 + [(500, 700, 300)] + [(300, 900, 40)] + [(2, 5, 9)] * 10, 4)])
    F.add("ml_131072_single", [("raw", b"Q"), comp([(0, 131072, 4)], 0)], block_max=131072)
    F.add("ml_131074_single", [("raw", b"Q"), comp([(0, 131074, 4)], 0)], B)
    F.add("ll_65536_code35", [("comp", lit("raw", T(70000)), seq([(65536 + 4000, 10, 8)]))])

    # ---- overlap and in-batch dependence ----
    for o in (1, 2, 3, 7, 8, 9):
        F.add("overlap_off%d" % o, [comp([(12, 3 * o + 5, o + 3), (1, 70 + o, o + 3), (0, max(3, o + 1), o + 3)], 1)])
        F.add("overlap_off%d_eq_ml" % o, [comp([(80, max(o, 3), max(o, 3) + 3), (1, 64 + o, 64 + o + 3)], 1)])
    F.add("chain_64", [comp([(8, 6, 9)] + [(0, 6, 9)] * 70, 1)])          # every match reads the one before it
    F.add("chain_64_lits", [comp([(8, 5, 9)] + [(1, 5, 8)] * 70, 1)])
    F.add("span_prev_batch", [comp([(4, 4, 6)] * 64 + [(0, 60, 30 + 3), (1, 65, 40 + 3)], 0)])
    F.add("span_prev_block", [comp([(40, 10, 23)], 3), comp([(2, 30, 15 + 3), (0, 70, 20 + 3)], 1)])

    # ---- repeat offsets ----
    for c in (1, 2, 3):
        F.add("rep_code%d_ll" % c, [comp([(30, 5, 13), (2, 4, 23), (3, 6, 10), (4, 7, c), (1, 5, c)], 1)])
        if c < 3:
            F.add("rep_code%d_ll0" % c, [comp([(30, 5, 13), (2, 4, 23), (3, 6, 10), (0, 7, c), (0, 5, c)], 1)])
        F.add("rep_first_code%d" % c, [comp([(12, 5, c)], 2)])               # history 1, 4, 8
        if c < 3:
            F.add("rep_first_code%d_ll0" % c, [("raw", T(9)), comp([(0, 5, c), (0, 4, c)], 2)])
    F.add("rep_code3_ll0", [comp([(30, 5, 13), (2, 4, 23), (3, 6, 10), (0, 7, 3), (0, 5, 3)], 1)])  # rep0 - 1 twice
    F.add("rep_first_code3_ll0_after_new", [("raw", T(9)), comp([(0, 5, 8), (0, 4, 3)], 2)])
    for k in (63, 64, 65):
        for c in (1, 2, 3):
            seqs = [(9, 4, 9 + 3)] + [(i % 3, 4, 3 + 4 + i % 9) for i in range(1, k - 1)] + [(c % 2, 5, c), (2, 4, 2)]
            F.add("rep_seq%d_code%d" % (k, c), [comp(seqs, 1)])
    for run in (1, 2, 3, 4):
        seqs = [(20, 4, 3 + 5), (1, 4, 2)]
        for r in range(6):
            seqs += [(1 + j, 4, 3 + 6 + j + r) for j in range(run)] + [(r % 2, 5, 1 + r % 3)]
        F.add("rep_run_%d_new" % run, [comp(seqs, 1)])
    F.add("rep_across_blocks", [comp([(20, 4, 3 + 5), (2, 4, 3 + 11), (2, 4, 3 + 17)], 1), ("raw", T(13)),
                                comp([(2, 5, 3), (1, 4, 2)], 0), ("rle", 0x41, 30), comp([(0, 4, 2), (0, 6, 1)], 2),
                                ("comp", lit("raw", T(5)), seq([])), comp([(1, 4, 3)], 0)])
    F.add("rep_rep0_minus1_zero", [("raw", T(9)), comp([(0, 5, 3)], 2)], B)   # rep0 = 1: 1 - 1 = 0
    F.add("rep_rep0_minus1_zero_later", [comp([(9, 5, 1 + 3), (0, 5, 3)], 2)], B)
    F.add("rep_alternate_2_3", [comp([(20, 4, 3 + 5), (2, 4, 3 + 11), (2, 4, 3 + 17)] +
                                     [(0 if i % 10 == 0 else 1, 4, 2 + i % 2) for i in range(200)], 1)])

    # ---- offsets against the start ----
    F.add("off_eq_position", [comp([(10, 5, 10 + 3)], 1)])
    F.add("off_position_plus1", [comp([(10, 5, 11 + 3)], 1)], B)
    F.add("off_eq_position_block2", [("raw", T(50)), comp([(10, 5, 60 + 3)], 1)])
    F.add("off_position_plus1_block2", [("raw", T(50)), comp([(10, 5, 61 + 3)], 1)], B)
    for c in range(17, 23):
        # the first offset of the code, from a position that makes it reach byte 0 of the frame; code 22 fills 4 MiB
        n = (1 << c) - 3 - 6
        h = [("rle", 0x20 + c, min(131072, n - i)) for i in range(0, n, 131072)]
        more = [(0, 5, (1 << c) + 3)] if c < 22 else []
        F.add("off_code%d_rle_history" % c, h + [comp([(6, 3, 1 << c)] + more, 0, of=("fse", 5))],
              window=(c - 10 + 1, 0), fcs=4)
    F.add("off_code31", [comp([(10, 5, (1 << 31) + 9)], 1, of="rle")], B)
    F.add("off_code32", [("comp", rawlit([(10, 5, 9)], 1), seq([(10, 5, 9)], of="rle",
                                                               desc=lambda t, d: bytes([32]) if t == 1 else d))], None)
    # beyond the window, inside the content: window 1 KiB, offset 3000 of 4000 bytes before it
    F.add("off_beyond_window", [("raw", T(1000))] * 4 + [comp([(4, 8, 3000 + 3)], 0)], None, window=(0, 0), fcs=0)

    # ---- sizes ----
    F.add("lits_exact", [comp([(5, 6, 7), (4, 4, 5)], 0)])
    F.add("lits_left", [comp([(5, 6, 7), (4, 4, 5)], 17)])
    F.add("lits_short", [("comp", lit("raw", T(8)), seq([(5, 6, 7), (4, 4, 5)]))], B)
    F.add("out_block_max", [comp([(100, 131072 - 100 - 7, 90 + 3)], 7)])
    F.add("out_block_max_plus1", [comp([(100, 131072 - 100 - 7, 90 + 3)], 8)], B)
    F.add("window_1k_block_at", [("raw", T(1024)), comp([(24, 1000, 20 + 3)], 0)], window=(0, 0), fcs=0,
          block_max=1024)
    F.add("window_1k_block_over", [("raw", T(1024)), comp([(24, 1000, 20 + 3)], 1)], B, window=(0, 0), fcs=0,
          block_max=1024)
    F.add("window_1k_raw_over", [("raw", T(1025))], B, window=(0, 0), fcs=0, block_max=1024)
    F.add("fcs_one_short", [comp([(10, 20, 8)], 3)], ST_SIZE_MISMATCH, "frame", content_size=34, fcs=4)
    F.add("fcs_one_long", [comp([(10, 20, 8)], 3)], None, "frame", content_size=32, fcs=4)

    # ---- literals ----
    for sf, n in ((0, 31), (2, 17), (1, 4095), (3, 4096), (3, 40), (1, 5)):
        F.add("lit_raw_sf%d_%d" % (sf, n), [("comp", lit("raw", T(n), sf=sf), seq([(3, 5, 6)]))])
        F.add("lit_rle_sf%d_%d" % (sf, n), [("comp", lit("rle", b"x" * n, sf=sf), seq([(3, 5, 4)]))])
    F.add("lit_rle_131072", [("comp", lit("rle", b"y" * 131072), seq([]))])
    sk = F.skew(40000)
    for n in (2, 1023):
        F.add("huf1_%d" % n, [("comp", lit("huf", sk[:n] if n > 2 else b"ab", streams=1), seq([(1, 3, 4)]))])
    F.add("huf1_1", [("comp", lit("huf", b"a", weights=[0] * 97 + [1, 1], streams=1), seq([]))])
    for n in (4, 6, 7, 8, 1023, 1024, 16383, 16384):
        F.add("huf4_%d" % n, [("comp", lit("huf", sk[:n], weights=huf_weights(sk), streams=4), seq([(2, 3, 5)]))])
    # 5 bytes in four streams: the first three hold (5 + 3) / 4 = 2 each, which leaves the fourth less than nothing
    F.add("huf4_5", [("comp", lit("huf", sk[:5], weights=huf_weights(sk), streams=4), seq([(2, 3, 5)]))], B)
    F.add("huf4_1023_sf2", [("comp", lit("huf", sk[:1023], streams=4, sf=2), seq([(2, 3, 5)]))])
    F.add("huf4_5byte_header", [("comp", lit("huf", sk[:300], streams=4, sf=3), seq([(2, 3, 5)]))])
    F.add("huf4_40000", [("comp", lit("huf", sk, streams=4), seq([(2, 3, 5)] + [(9, 4, 14)] * 30))])
    # 11-bit codes: a chain over 14 symbols, the two rarest 11 bits long; streams of 127 / 128 / 129 of them
    w11 = [0] * 65 + [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    assert max(l for _, l in huf_codes(w11).values()) == 11
    rare = [s for s, (_, l) in huf_codes(w11).items() if l == 11]
    for n in (127, 128, 129, 300):
        d = bytes(rare[i % 2] for i in range(n))
        F.add("huf1_11bit_%d" % n, [("comp", lit("huf", d, weights=w11, streams=1), seq([(2, 3, 4)]))])
        F.add("huf4_11bit_%d" % n, [("comp", lit("huf", d * 4 + d[:3], weights=w11, streams=4), seq([(2, 3, 4)]))])
    F.add("huf_maxbits11_derived", [("comp", lit("huf", F.skew(6000, 60), maxbits=11, exact_max=True), seq([(2, 3, 5)]))])
    F.add("huf_direct_2", [("comp", lit("huf", bytes([0, 1] * 40 + [1]), weights=[1, 1], streams=1), seq([(2, 3, 4)]))])
    w127 = [1] * 128          # 127 written + the implied one: 128 symbols of 7 bits
    F.add("huf_direct_127", [("comp", lit("huf", bytes(F.rng.randrange(128) for _ in range(700)), weights=w127,
                                          streams=1), seq([(2, 3, 4)]))])
    w128 = [2] * 127 + [1, 1]  # 128 written + the implied one
    F.add("huf_direct_128", [("comp", lit("huf", bytes(F.rng.randrange(129) for _ in range(700)), weights=w128,
                                          streams=4), seq([(2, 3, 4)]))])
    for nsym in (129, 200, 255, 256):
        d = bytes(F.rng.choices(range(nsym), [3 + (i * 7) % 13 for i in range(nsym)], k=5000)) + bytes(range(nsym))
        F.add("huf_fse_weights_%d" % nsym, [("comp", lit("huf", d, fse=True), seq([(2, 3, 5)]))])
    F.add("huf_fse_weights_few", [("comp", lit("huf", sk[:900], fse=True, streams=1), seq([(2, 3, 5)]))])
    # rejected trees.  12 bits: weights 1,1,2,...,11 written, the implied one is 12
    w12 = [1, 1] + list(range(2, 12)) + [12]
    F.add("huf_bad_12bit", [("comp", lit("huf", bytes([12] * 20), weights=w12, streams=1), seq([]))], B)
    F.add("huf_bad_one_weight", [("comp", lit("huf", b"\x01" * 9, weights=[0, 1], streams=1,
                                              tree=bytes([128, 0x00]), streams_bytes=[b"\x01\x01"]), seq([]))], B)
    F.add("huf_bad_remainder", [("comp", lit("huf", b"\x00" * 9, weights=[2, 1, 1], streams=1,
                                             tree=bytes([127 + 3, 0x21, 0x10]), streams_bytes=[b"\x01\x01"]), seq([]))], B)
    good = huf_stream(sk[:200], huf_codes(huf_weights(sk)))
    F.add("huf_bad_stream_not_at_0", [("comp", lit("huf", sk[:199], weights=huf_weights(sk), streams=1,
                                                   streams_bytes=[good]), seq([]))], B)
    F.add("huf_bad_stream_last_byte_0", [("comp", lit("huf", sk[:200], weights=huf_weights(sk), streams=1,
                                                      streams_bytes=[good + b"\0"]), seq([]))], B)
    F.add("huf_bad_jump_overrun", [("comp", lit("huf", sk[:400], weights=huf_weights(sk), streams=4,
                                                jump=(100, 100, 600)), seq([]))], B)
    F.add("huf_bad_treeless_first", [("bytes", bytes([3 | 0 << 2 | (4 << 4) & 0xFF, (4 >> 4) | (2 << 6) & 0xFF, 0,
                                                      0x5, 0x1, 0]), 2)], B)
    hb = ("comp", lit("huf", sk[:500], weights=huf_weights(sk)), seq([(2, 3, 5)]))
    tl = lambda n, k: ("comp", lit("treeless", sk[k:k + n]), seq([(2, 3, 5)]))  # noqa: E731
    F.add("huf_treeless", [hb, tl(300, 500), tl(2000, 900)])
    F.add("huf_treeless_after_rawlit", [hb, comp([(3, 4, 8)], 3), tl(300, 500)])
    F.add("huf_treeless_after_raw_rle", [hb, ("raw", T(30)), ("rle", 9, 40), tl(300, 500)])

    # ---- sequence tables ----
    mixed = [(i % 7, 3 + i % 5, 4 + i % 9) for i in range(1, 60)]
    same = [(4, 5, 6 + i % 2) for i in range(20)]
    for t, key in enumerate(("ll", "of", "ml")):
        F.add("tab_%s_fse" % key, [comp([(9, 4, 5)] + mixed, 1, **{key: ("fse", 5 if t == 1 else 6)})])
        vary = [(4 if t == 0 else 3 + i % 6, 5 if t == 2 else 3 + i % 7, 6 if t == 1 else 4 + i % 9) for i in range(25)]
        F.add("tab_%s_rle" % key, [("raw", T(20)), comp(vary, 1, **{key: "rle"})])
        F.add("tab_%s_rep" % key, [comp([(9, 4, 5)] + mixed, 1, **{key: ("fse", 5)}),
                                   comp(mixed, 1, **{key: "rep"})])
    allfse = lambda a, b, c, **k: dict(ll=("fse", a), of=("fse", b), ml=("fse", c), **k)  # noqa: E731
    wide = [(9, 4, 5)] + [(i % 30, 3 + i % 40, 4 + i % 250) for i in range(1, 400)]
    for als in ((5, 5, 5), (6, 5, 6), (7, 7, 7), (9, 8, 9)):
        F.add("tab_al_%d_%d_%d" % als, [comp(wide if als[0] > 5 else [(9, 4, 5)] + mixed * 3, 1, **allfse(*als))])

    def al_byte(table, al):
        return lambda t, d: bytes([(d[0] & 0xF0) | (al - 5)]) + d[1:] if t == table else d
    for t, key in enumerate(("ll", "of", "ml")):
        F.add("tab_bad_al_%s_%d" % (key, MAX_AL[t] + 1), [comp(wide, 1, **allfse(9, 8, 9, desc=al_byte(t, MAX_AL[t] + 1)))], B)
    F.add("tab_minus1", [comp(wide, 1, ll=("fse", 7, None, "minus1"), of=("fse", 7, None, "minus1"),
                              ml=("fse", 7, None, "minus1"))])
    # zero runs: codes 0 and 4, 0 and 8 (3 + 3 + 1: a 3, 3 chain), 0 and 11 (3, 3, 3 chain then 0), 0 and 1 (flag 0)
    for gap in (1, 2, 4, 7, 8, 10, 11, 13, 30):
        seqs = [(6, 4, 5)] + [(0 if i % 2 else gap, 3 if i % 3 else 3 + gap, 4) for i in range(1, 40)]
        F.add("tab_zero_run_%d" % gap, [comp(seqs, 1, ll=("fse", 5), ml=("fse", 5))])
    # a description that ends mid-byte: the bitstream starts at the next whole byte
    mb = [(9, 4, 5)] + mixed
    hist = [0] * 16
    for a, _, _ in mb:
        hist[ll_code(a)] += 1
    nm = normalize(hist, 6)
    assert fse_describe(nm, 6).n % 8 != 0
    F.add("tab_desc_ends_mid_byte", [comp(mb, 1, ll=("fse", 6, nm))])
    F.add("tab_bad_ll_sym_36", [comp(same, 0, ll="rle", desc=lambda t, d: bytes([36]) if t == 0 else d)], B)
    F.add("tab_bad_of_sym_32", [comp(same, 0, of="rle", ml="rle", desc=lambda t, d: bytes([32]) if t == 1 else d)], None)
    F.add("tab_bad_ml_sym_53", [comp([(4, 5, 6)] * 20, 0, ml="rle", desc=lambda t, d: bytes([53]) if t == 2 else d)], B)
    # a compressed description that names symbol 36 / 53: counts over one symbol more than the alphabet
    nl = [2] * 4 + [0] * 32 + [24]
    F.add("tab_bad_ll_fse_sym_36", [comp([(1, 5, 6)] * 20, 0, ll=("fse", 5, nl))], B)
    F.add("tab_bad_rep_first", [("bytes", bytes([1 << 3, 0x41, 1, 0xFC, 0x01]), 2)], B)
    for key, first in (("pre", {}), ("rle", dict(ll="rle", of="rle", ml="rle")), ("fse", allfse(6, 5, 6))):
        s0 = [(4, 5, 6)] * 30 if key == "rle" else [(9, 4, 5)] + mixed
        F.add("tab_rep_after_%s" % key, [comp(s0, 1, **first), comp(s0[1:], 1, ll="rep", of="rep", ml="rep")])
    F.add("tab_rep_over_nseq0", [comp([(9, 4, 5)] + mixed, 1, **allfse(6, 5, 6)), ("comp", lit("raw", T(9)), seq([])),
                                 ("raw", T(3)), comp(mixed, 1, ll="rep", of="rep", ml="rep")])
    F.add("tab_small_then_general", [comp([(9, 4, 5)] + mixed, 1, **allfse(6, 5, 6)), comp(mixed, 1),
                                     comp(mixed, 1, ll="rep", of="rep", ml="rep"), comp(wide, 1, **allfse(9, 8, 9)),
                                     comp(wide[1:], 1, ll="rep", of="rep", ml="rep"), comp(mixed, 1, **allfse(6, 5, 6))])
    g = F.skew(7000, 60)
    F.add("tab_general_huf", [("comp", lit("huf", g, exact_max=True), seq(wide, **allfse(7, 6, 7))),
                              ("comp", lit("treeless", g[500:6900]), seq(wide[1:], ll="rep", of="rep", ml="rep"))])
    F.add("seq_bad_last_byte_0", [comp([(9, 4, 5)] + mixed, 1, bits=lambda b: b + b"\0")], B)

    def one_bit_short(b):
        v = int.from_bytes(b, "little")
        top = v.bit_length() - 1                 # the marker; drop the first bit the decoder reads and move it down
        v = (v & ((1 << (top - 1)) - 1)) | 1 << (top - 1)
        return v.to_bytes((top + 7) // 8, "little")
    F.add("seq_bad_one_bit_short", [comp([(9, 4, 5)] + mixed, 1, bits=one_bit_short)], B)
    F.add("seq_bad_one_byte_long", [comp([(9, 4, 5)] + mixed, 1, bits=lambda b: b"\0" + b)], B)
    F.add("seq_bad_nseq0_trailing", [("comp", lit("raw", T(9)), seq([], tail=b"\0"))], B)
    F.add("seq_bad_modes_reserved", [comp([(9, 4, 5)] + mixed, 1, modes=1)], B)

    # ---- frames the sequence pre-pass of the record decoder takes (zstd_dec_seq.hip): more than 128 KiB of content, two
    # blocks with sequences, the second with tables of its own.  The sequences under test sit in that second block behind
    # one sequence that pins the history to 37, 7, 9.  Its scratch holds one sequence per 8 bytes of content, so the blocks
    # with the most sequences sit behind 384 KiB of RLE history ----
    filler = [(9, 4, 7 + 3)] + [(i % 5, 3 + i % 4, 9 + 3) for i in range(30)]

    def sp(name, seqs, status=ST_OK, third=None, pin=True, nhist=1, **sk):
        m = dict(allfse(6, 5, 6))
        m.update(sk)
        blocks = hist128k * nhist + [comp(filler, 2, **allfse(6, 5, 6)), comp(([(11, 7, 37 + 3)] if pin else []) + seqs, 3, **m)]
        if third:
            blocks.append(comp(third, 1, ll="rep", of="rep", ml="rep"))
        F.add("sp_" + name, blocks, status)
    for c in (1, 2, 3):
        sp("rep_code%d_ll" % c, [(2, 4, 23), (3, 6, 10), (4, 7, c), (1, 5, c), (2, 4, c)])
        sp("rep_code%d_ll0" % c, [(2, 4, 23), (3, 6, 10), (0, 7, c), (0, 5, c), (2, 4, 3)])
        for k in (63, 64, 65):
            seqs = [(i % 3, 4, 3 + 4 + i % 9) for i in range(1, k - 1)] + [(c % 2, 5, c), (2, 4, 2), (0, 3, 3)]
            sp("rep_seq%d_code%d" % (k, c), seqs)
    for run in (1, 2, 3, 4):
        seqs = [(1, 4, 2)]
        for r in range(8):
            seqs += [(1 + j, 4, 3 + 6 + j + r) for j in range(run)] + [(r % 2, 5, 1 + r % 3)]
        sp("rep_run_%d_new" % run, seqs, third=[(0, 4, 2), (1, 5, 3), (0, 4, 1)])
    sp("rep_alternate_2_3", [(2, 4, 3 + 11), (2, 4, 3 + 17)] + [(0 if i % 10 == 0 else 1, 4, 2 + i % 2) for i in range(200)])
    sp("rep_rep0_minus1_zero", [(3, 4, 1 + 3), (0, 5, 3)], B)
    for n in (63, 64, 65, 129):
        sp("batch_%d" % n, [(i % 3, 3 + i % 6, 4 + i % 11) for i in range(1, n)])
    sp("chain_64", [(0, 6, 9)] * 70)
    sp("long_mid_batch", [(3, 5, 6)] * 30 + [(2000, 4000, 1000)] + [(2, 5, 9)] * 50, ll=("fse", 5), ml=("fse", 5))
    sp("pack_ml_131000", [(0, 131000, 4)], pin=False, ll="rle", of="rle", ml="rle")
    sp("pack_ll_65600_ml_65500", [(65600 - 11, 20, 9)], third=None, pin=False, ll="rle", of="rle", ml="rle")
    sp("nseq_0x7EFF", [(0, 3, 4 + i % 3 * 3) for i in range(0x7EFF)], pin=False, nhist=3, of=("fse", 5), ll="rle", ml=("fse", 5))
    sp("nseq_0x7F00", [(0, 3, 4 + i % 3 * 3) for i in range(0x7F00)], pin=False, nhist=3, of=("fse", 5), ll="rle", ml=("fse", 5))
    sp("nseq_above_block_max_4", [(0, 3, 4 + (i % 4)) for i in range(36000)], pin=False, nhist=3, of=("fse", 5), ll="rle", ml=("fse", 5))

    # ---- unit look-alikes: what the device encoder writes is a Huffman or raw-literals head block and treeless / raw
    # followers, all Predefined or head-describes-rest-repeats; each of these differs in one thing ----
    u = F.skew(200000, 30)
    useq = [(20 + i % 9, 6 + i % 5, 4 + 9 + i % 60) for i in range(60)]
    ulen = sum(a for a, _, _ in useq)
    uw = huf_weights(u)

    def ub(kind, at, n=None, first=False, **sk):
        n = n if n is not None else ulen + 40
        m = dict(allfse(6, 5, 6)) if first else dict(ll="rep", of="rep", ml="rep")
        m.update(sk)
        return ("comp", lit(kind, u[at:at + n], streams=4, weights=uw), seq(useq, **m))
    F.add("unit_plain", [ub("huf", 0, first=True)] + [ub("treeless", 3000 * i) for i in range(1, 5)])
    F.add("unit_follower_own_tree", [ub("huf", 0, first=True), ub("treeless", 3000), ub("huf", 6000), ub("treeless", 9000)])
    F.add("unit_follower_other_modes", [ub("huf", 0, first=True), ub("treeless", 3000),
                                        ub("treeless", 6000, ll="pre", of="rep", ml="rep"), ub("treeless", 9000)])
    F.add("unit_follower_predefined", [ub("huf", 0, first=True, ll="pre", of="pre", ml="pre")] +
          [ub("treeless", 3000 * i, ll="pre", of="pre", ml="pre") for i in range(1, 4)])
    for k in (16, 17):
        F.add("unit_%d_followers" % k, [ub("huf", 0, first=True)] + [ub("treeless", 2000 * i) for i in range(1, k + 1)])
    F.add("unit_raw_head", [("comp", lit("raw", T(ulen + 9)), seq(useq, **allfse(6, 5, 6)))] +
          [("comp", lit("raw", T(ulen + 9)), seq(useq, ll="rep", of="rep", ml="rep")) for _ in range(3)])
    # four streams need the 6-byte jump table and a byte each: a compressed size of 9 cannot hold them
    tiny = ("comp", lit("treeless", u[:30], streams=4, weights=uw, streams_bytes=[b"\x01", b"\x01", b"\x01", b""]),
            seq(useq[:1], ll="rep", of="rep", ml="rep"))
    F.add("unit_follower_csz_below_10", [ub("huf", 0, first=True), tiny, ub("treeless", 6000)], B)
    F.add("unit_follower_csz_10", [ub("huf", 0, first=True), ("comp", lit("treeless", u[:4] + u[:20], streams=4, weights=uw, sf=1),
                                                               seq(useq[:1], ll="rep", of="rep", ml="rep")), ub("treeless", 6000)])
    big = seq([(20, 6, 13)] * 3, **allfse(5, 5, 5))
    for name, extra in (("under", -1), ("over", 1)):
        # head + followers whose regenerated literal sizes add up to one byte under / over 128 KiB
        sizes = [30000, 30000, 30000, 30000, 131072 - 120000 + extra]
        at, blocks = 0, []
        for i, n in enumerate(sizes):
            blocks.append(("comp", lit("huf" if i == 0 else "treeless", u[at:at + n], streams=4, weights=uw),
                           big if i == 0 else seq([(20, 6, 13)] * 3, ll="rep", of="rep", ml="rep")))
            at += n
        F.add("unit_regen_128k_%s" % name, blocks)

    # ---- frame headers ----
    body = [comp([(10, 20, 8)], 3)]
    for n, size in ((0, None), (1, None), (2, 300), (4, None), (8, None)):
        F.add("hdr_fcs%d" % n, body if size is None else [("raw", T(size))], fcs=n, single=(n == 1))
    F.add("hdr_single_block_above_window", [("comp", lit("raw", T(40)), seq([]))], B, fcs=1, single=True)
    F.add("hdr_fcs2_single", [("raw", T(256))], fcs=2, single=True)
    F.add("hdr_fcs2_max", [("raw", T(65535 + 256))], fcs=2, single=True)
    F.add("hdr_fcs4_single", body, fcs=4, single=True)
    F.add("hdr_fcs8_single", body, fcs=8, single=True)
    F.add("hdr_window_e0_m0", body, fcs=4, window=(0, 0))
    F.add("hdr_window_e5_m7", body, fcs=4, window=(5, 7))
    F.add("hdr_window_e21_m7", body, fcs=4, window=(21, 7))
    for w in (1, 2, 4):
        F.add("hdr_did%d_zero" % w, body, fcs=4, did_width=w, did=0)
    F.add("hdr_did4_nonzero", body, None, "frame", fcs=4, did_width=4, did=0x12345678)
    F.add("hdr_did1_nonzero", body, None, "frame", fcs=4, did_width=1, did=7)
    F.add("hdr_reserved_bit", body, ST_BAD_FRAME, "frame", fcs=4, reserved=1)
    F.add("hdr_unused_bit", body, fcs=4, unused=1)
    F.add("hdr_checksum", body, fcs=4, checksum=True)
    F.add("hdr_checksum_nofcs", body + [("raw", T(700))], fcs=0, checksum=True)
    F.add("hdr_checksum_wrong", body, ST_BAD_CHECKSUM, "frame", fcs=4, checksum=0x12345678)
    F.add("hdr_empty_frame", [("raw", b"")])
    F.add("hdr_empty_frame_nofcs", [("raw", b"")], fcs=0)
    F.add("hdr_empty_raw_last", body + [("raw", b"")])
    F.add("hdr_empty_rle_last", body + [("rle", 7, 0)])
    F.add("hdr_block_type3", [("bytes", b"abcd", 3)], B)
    F.add("hdr_block_type3_later", body + [("bytes", b"abcd", 3)], B)
    F.add("hdr_comp_block_size_0", [("bytes", b"", 2)], B)
    assert not F.bad, F.bad
    return F.cases


def content_size_field(fr: bytes):
    """the Frame_Content_Size a frame states, None without the field"""
    fhd = fr[4]
    single, fl, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    n = ((1 if single else 0), 2, 4, 8)[fl]
    if not n:
        return None
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[did]
    return int.from_bytes(fr[at:at + n], "little") + (256 if fl == 1 else 0)
