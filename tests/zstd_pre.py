"""Helpers of the entropy pre-pass tests (TEST CODE ONLY): a header walk of its own that says which blocks
gpumt_zstd_decompress_blocks_pre must mark, the emulated call, the comparison of two carries, and the cases that
tests/test_emu_zstd_plain_pre.py and tests/test_gpu_zstd_plain_pre.py share."""
import ctypes as C
import functools
import os
import struct

import numpy as np

import helpers as H
import zstd_blocks as Z
from golden import cases
from zstdmt_amd.device import ZSTD_BLOCK, ZSTD_RUN, ZSTD_CARRY_BYTES

SEQ, LIT = 1, 2                       # mark bits
FIXTURE_NAMES = sorted(os.path.splitext(f)[0] for f in os.listdir(Z.FIX_DIR) if f.endswith(".zst"))


# ---- the header walk ----------------------------------------------------------------------------------------------------
def sections(raw: bytes):
    """one Compressed_Block with its 3-byte header -> dict(lit_type, lit_hdr (offset, length in raw), regen, nseq, modes,
    seq_hdr (offset, length: Number_of_Sequences and the modes byte)); RFC 8878 3.1.1.3"""
    body = raw[3:]
    b0 = body[0]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt < 2:
        hl = (1, 2, 1, 3)[sf]
        regen = int.from_bytes(body[:hl], "little") >> (3 if hl == 1 else 4)
        csz = regen if lt == 0 else 1
    else:
        hl, bits = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
        v = int.from_bytes(body[:hl], "little")
        regen, csz = (v >> 4) & ((1 << bits) - 1), (v >> (4 + bits)) & ((1 << bits) - 1)
    sq = hl + csz
    n, p = body[sq], 1
    if n == 255:
        n, p = int.from_bytes(body[sq + 1:sq + 3], "little") + 0x7F00, 3
    elif n >= 128:
        n, p = ((n - 128) << 8) + body[sq + 1], 2
    modes = body[sq + p] if n else None
    return dict(lit_type=lt, lit_hdr=(3, hl), regen=regen, nseq=n, modes=modes, seq_hdr=(3 + sq, p + (1 if n else 0)))


def expected_marks(info, lo, hi):
    """blocks [lo, hi) of the frame as one run of one call -> the mark every block must get: bit 1 (literals) for a
    Compressed block with raw, RLE or Huffman literals whose tree is its own or a block's of [lo, its index); bit 0
    (sequences) when it has no sequences, or at most block_max / 4 and every Repeat_Mode table was last described by a
    block of [lo, its index); 0 for Raw and RLE blocks"""
    out, tree, tab = [], False, [False, False, False]
    for b in info["blocks"][lo:hi]:
        if b["type"] != 2:
            out.append(0)
            continue
        s, m = sections(b["raw"]), 0
        if s["lit_type"] == 2:
            tree = True
        if s["lit_type"] < 2 or tree:
            m |= LIT
        if s["nseq"] == 0:
            m |= SEQ
        else:
            mode = [(s["modes"] >> sh) & 3 for sh in (6, 4, 2)]
            if all(mode[t] != 3 or tab[t] for t in range(3)) and s["nseq"] <= info["block_max"] // 4:
                m |= SEQ
            tab = [tab[t] or mode[t] != 3 for t in range(3)]
        out.append(m)
    return out


def fixture_kinds():
    """what the blocks of the committed streams take from earlier blocks, over all of them"""
    kinds = set()
    for name in FIXTURE_NAMES:
        for b in Z.walk(Z.fixture(name)[0])["blocks"]:
            if b["type"] == 2:
                s = sections(b["raw"])
                if s["lit_type"] == 3:
                    kinds.add("treeless")
                if s["nseq"]:
                    kinds |= {"repeat_" + k for k, sh in (("ll", 6), ("of", 4), ("ml", 2)) if (s["modes"] >> sh) & 3 == 3}
    return kinds


# ---- the carry ----------------------------------------------------------------------------------------------------------
def carry_state(cy: bytes, slot):
    """what a carry slot says: the 15 state words and, of each table, the cells a decoder can reach -- 2^log of them when
    the table is there.  The cells above are never read (an FSE state and a Huffman index are below 2^log); they hold
    whatever an earlier, larger table or the start of the kernel left in the wave's LDS, which two launches of the same
    serial kernel do not share either.  This asks less than equal carry bytes: it is every byte a later call can read."""
    at = slot * ZSTD_CARRY_BYTES
    w = struct.unpack_from("<15I", cy, at)
    rep, huf_ok, huf_log, tab_ok, tab_log, tab_pre, corrupt = w[0:3], w[3], w[4], w[5:8], w[8:11], w[11:14], w[14]
    out = [rep, huf_ok, tab_ok, tab_pre, corrupt]
    at += 64
    if huf_ok:
        out += [huf_log, cy[at:at + 2 * (1 << huf_log)]]
    at += 2 * 2048
    for t, cells in enumerate((512, 256, 512)):
        if tab_ok[t]:
            out += [tab_log[t], cy[at:at + 4 * (1 << tab_log[t])]]
        at += 4 * cells
    return out


# ---- the emulated call --------------------------------------------------------------------------------------------------
def emu_decode_blocks_pre(stream, blocks, runs, out_bytes, history=b"", carry=None, pre_on=1):
    """emu_zstd_decompress_blocks_pre with Engine.zstd_decompress_blocks_pre's shape -> (output area, run_len, status,
    carry, mark)"""
    import emu_driver as E
    L = E.lib()
    nblk, nrun = len(blocks), len(runs)
    sbuf = np.frombuffer(bytes(stream) + b"\xEE" * 320, np.uint8).copy()
    area = np.full(out_bytes + 64, 0xCC, np.uint8)
    area[:len(history)] = np.frombuffer(history, np.uint8)
    cy = np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8) if carry is None else np.frombuffer(carry, np.uint8).copy()
    rl, st = np.full(nrun, 0xA5A5A5A5, np.uint32), np.full(nrun, 99, np.uint32)
    mk = np.full(nblk, 0xA5A5A5A5, np.uint32)
    blocks, runs = np.ascontiguousarray(blocks, ZSTD_BLOCK), np.ascontiguousarray(runs, ZSTD_RUN)
    L.emu_zstd_decompress_blocks_pre(E._p(sbuf), C.c_uint64(len(stream)), E._p(blocks), C.c_uint32(nblk), E._p(runs),
                                     C.c_uint32(nrun), E._p(area), C.c_uint64(out_bytes), E._p(cy), E._p(rl), E._p(st),
                                     E._p(mk), C.c_int(pre_on))
    assert (area[out_bytes:] == 0xCC).all(), "decoder wrote past the end of its output"
    return area[:out_bytes].tobytes(), rl, st, cy.tobytes(), mk


# ---- cases --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame(name):
    """-> (frame bytes, content, walk) of a committed stream, or of "hand": raw, RLE and empty blocks among compressed ones
    with raw literals and RLE-mode tables"""
    if name == "hand":
        a, b, lits = cases.text(3000, 71), cases.rnd(700, 72), cases.text(20, 73)
        blocks = [("raw", a), ("cooked", Z.match_block(lits, 3000, 30)), ("rle", 0x41, 500), ("raw", b),
                  ("cooked", Z.match_block(lits, 4100, 30)), ("raw", b"")]
        plain = a + lits + a[20:50]
        plain += b"\x41" * 500 + b + lits
        plain += plain[len(plain) - 4100:len(plain) - 4100 + 30]
        fr = Z.frame_of(blocks, csize=len(plain))
    else:
        fr, plain = Z.fixture(name)
    return fr, plain, Z.walk(fr)


def cut_params():
    """(frame, cut): cut 0 = the frame as one run, cut k = two calls with the boundary in front of block k"""
    return [(n, k) for n in FIXTURE_NAMES + ["hand"] for k in range(len(frame(n)[2]["blocks"]))]


def decode_parts(dec, info, cut):
    """the frame through `dec` (a decode function, 4 or 5 results) as one call (cut 0) or two -> list per call of
    (output of the call, run_len, status, carry state left (None behind the last call), mark list or None)"""
    n, res = len(info["blocks"]), []
    bounds = [(0, n)] if cut == 0 else [(0, cut), (cut, n)]
    hist_bytes, cy = b"", None
    for lo, hi in bounds:
        hist = min(len(hist_bytes), info["window"])
        s, b, r, o = Z.tables(info, lo, hi, hist=hist)
        got = dec(s, b, r, o, history=hist_bytes[len(hist_bytes) - hist:], carry=cy)
        out, rl, st, cy = got[:4]
        res.append((out[hist:hist + int(rl[0])], int(rl[0]), int(st[0]), carry_state(cy, 0) if hi < n else None,
                    [int(x) for x in got[4]] if len(got) > 4 else None))
        if int(st[0]) != 0:
            break
        hist_bytes += out[hist:hist + int(rl[0])]
    return res


_serial = {}


def serial_parts(dec, key, info, cut):
    """decode_parts through the serial entry point, computed once per (device kind, frame, cut)"""
    if key not in _serial:
        _serial[key] = decode_parts(dec, info, cut)
    return _serial[key]


SAMPLES = {"emu": 24, "gpu": 768}      # a flip costs about a second under the emulator and milliseconds on the device


def flips(info, nblk, group, count=24):
    """positions (offsets into the stream of blocks [0, nblk)) of the damage test, one bit each: group "headers" = every
    byte of the first block's block header, literals section header and sequences section header; "sample<i>" = every
    third of `count` positions spread evenly over the stream, starting at the i-th"""
    total = sum(len(b["raw"]) for b in info["blocks"][:nblk])
    if group == "headers":
        s = sections(info["blocks"][0]["raw"])
        pos = list(range(3)) + list(range(s["lit_hdr"][0], sum(s["lit_hdr"]))) + list(range(s["seq_hdr"][0], sum(s["seq_hdr"])))
    else:
        pos = [7 + k * (total - 8) // (count - 1) for k in range(count)][int(group[6:])::3]
    return [(p, 1 << (p % 8)) for p in pos]
