"""Helpers of the block-parallel execute stage tests (TEST CODE ONLY): the emulated gpumt_zstd_decompress_blocks_par, which
blocks it must report as decoded side by side, hand-built frames at the stage's edges (tests/zstd_synth.py) and the cases
that tests/test_emu_zstd_plain_par.py and tests/test_gpu_zstd_plain_par.py share."""
import ctypes as C
import functools

import numpy as np

import zstd_blocks as Z
import zstd_pre as P
import zstd_synth as S
from zstdmt_amd.device import ZSTD_BLOCK, ZSTD_RUN, ZSTD_CARRY_BYTES

FULL = P.SEQ | P.LIT


def emu_decode_blocks_par(stream, blocks, runs, out_bytes, history=b"", carry=None, par_on=1):
    """emu_zstd_decompress_blocks_par with Engine.zstd_decompress_blocks_par's shape -> (output area, run_len, status,
    carry, mark, par)"""
    import emu_driver as E
    L = E.lib()
    nblk, nrun = len(blocks), len(runs)
    sbuf = np.frombuffer(bytes(stream) + b"\xEE" * 320, np.uint8).copy()
    area = np.full(out_bytes + 64, 0xCC, np.uint8)
    area[:len(history)] = np.frombuffer(history, np.uint8)
    cy = np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8) if carry is None else np.frombuffer(carry, np.uint8).copy()
    rl, st = np.full(nrun, 0xA5A5A5A5, np.uint32), np.full(nrun, 99, np.uint32)
    mk, pr = np.full(nblk, 0xA5A5A5A5, np.uint32), np.full(nblk, 0xA5A5A5A5, np.uint32)
    blocks, runs = np.ascontiguousarray(blocks, ZSTD_BLOCK), np.ascontiguousarray(runs, ZSTD_RUN)
    L.emu_zstd_decompress_blocks_par(E._p(sbuf), C.c_uint64(len(stream)), E._p(blocks), C.c_uint32(nblk), E._p(runs),
                                     C.c_uint32(nrun), E._p(area), C.c_uint64(out_bytes), E._p(cy), E._p(rl), E._p(st),
                                     E._p(mk), E._p(pr), C.c_int(par_on))
    assert (area[out_bytes:] == 0xCC).all(), "decoder wrote past the end of its output"
    return area[:out_bytes].tobytes(), rl, st, cy.tobytes(), mk, pr


def expected_par(info, lo, hi):
    """blocks [lo, hi) as one run of one call -> (block_par list, blocks of the serial prefix): the suffix is everything
    behind the last Compressed block that is not fully marked; fewer than 2 blocks there leave the whole run serial"""
    marks, s = P.expected_marks(info, lo, hi), 0
    for i, b in enumerate(info["blocks"][lo:hi]):
        if b["type"] == 2 and marks[i] != FULL:
            s = i + 1
    n = hi - lo
    if n - s < 2:
        return [0] * n, n
    return [0] * s + [1] * (n - s), s


def decode_parts(decs, info, cut, cap_cut=None):
    """P.decode_parts with one decode function per call (serial, pre and par results differ in length: the fifth is the
    mark list, the sixth the par list) -> list per call of (bytes, run_len, status, carry state or None, marks, par)"""
    n, res = len(info["blocks"]), []
    bounds = [(0, n)] if cut == 0 else [(0, cut), (cut, n)]
    hist_bytes, cy = b"", None
    for dec, (lo, hi) in zip(decs, bounds):
        hist = min(len(hist_bytes), info["window"])
        s, b, r, o = Z.tables(info, lo, hi, hist=hist)
        got = dec(s, b, r, o, history=hist_bytes[len(hist_bytes) - hist:], carry=cy)
        out, rl, st, cy = got[:4]
        res.append((out[hist:hist + int(rl[0])], int(rl[0]), int(st[0]), P.carry_state(cy, 0) if hi < n else None,
                    [int(x) for x in got[4]] if len(got) > 4 else None, [int(x) for x in got[5]] if len(got) > 5 else None))
        if int(st[0]) != 0:
            break
        hist_bytes += out[hist:hist + int(rl[0])]
    return res


def thin(cuts):
    """every 4th cut plus the first and the last (the device tests)"""
    cuts = list(cuts)
    return sorted(set(cuts[::4] + cuts[:1] + cuts[-1:]))


# ---- hand-built frames ------------------------------------------------------------------------------------------------------
WINDOW = (0, 0)     # Window_Descriptor of 1 KiB = Block_Maximum_Size: a frame of 3..6 blocks is a few KiB


def _rnd(n, seed):
    from golden import cases
    return cases.rnd(n, seed)


def comp(lits, seqs):
    """a Compressed block with raw literals and predefined tables (fully marked): seqs = [(ll, ml, offset value)]"""
    return ("comp", S.lit("raw", lits), S.seq(seqs))


def hand_blocks():
    """name -> block list.  Offsets stay within the 1 KiB window, so every cut keeps the sources in its history."""
    R = _rnd
    c = {}
    # sources one, two and three blocks back
    c["back_1_2_3"] = [("raw", R(300, 1)), ("raw", R(300, 2)), ("raw", R(300, 3)),
                       comp(R(12, 4), [(2, 20, 3 + 150), (2, 20, 3 + 474), (2, 20, 3 + 800)]),
                       comp(R(12, 5), [(3, 9, 3 + 70), (1, 30, 3 + 400), (2, 64, 3 + 1000), (0, 70, 3 + 700)])]
    # a source that straddles the block's start (offset >= length), and one with offset < length
    c["straddle"] = [("raw", R(300, 6)), comp(R(30, 7), [(10, 12, 3 + 15), (3, 40, 3 + 30)]),
                     comp(R(30, 8), [(10, 12, 3 + 15), (2, 90, 3 + 19), (1, 5, 3 + 3)]), ("raw", R(50, 9))]
    # offset < match length, the first period wholly before the block's start
    c["period_before"] = [("raw", R(200, 10)), comp(R(10, 11), [(0, 40, 3 + 5), (0, 100, 3 + 1), (4, 80, 3 + 70)]),
                          comp(R(10, 12), [(0, 41, 3 + 7), (0, 200, 3 + 3)]), comp(R(8, 13), [(0, 66, 3 + 65)])]
    # a byte that arrives from outside and is copied three times inside the block
    c["copied_thrice"] = [("raw", R(300, 14)), comp(R(4, 15), [(0, 8, 3 + 100), (0, 8, 3 + 8), (0, 8, 3 + 8), (0, 8, 3 + 16)]),
                          comp(R(4, 16), [(0, 8, 3 + 30), (0, 8, 3 + 8), (0, 80, 3 + 16), (0, 8, 3 + 96), (2, 8, 3 + 50)])]
    # repeat codes at the start of a block: 1, 2, 3 with ll > 0 and with ll == 0 (the last being rep0 - 1)
    sets = comp(R(9, 17), [(3, 5, 3 + 100), (3, 5, 3 + 200), (3, 5, 3 + 300)])
    c["rep_ll_pos"] = [("raw", R(400, 18)), sets, comp(R(9, 19), [(1, 5, 1), (1, 5, 2), (1, 5, 3), (1, 6, 3 + 33), (1, 4, 2)]),
                       comp(R(9, 20), [(2, 5, 3), (2, 5, 2), (2, 5, 1)])]
    c["rep_ll_zero"] = [("raw", R(400, 21)), sets, comp(R(9, 22), [(0, 5, 1), (0, 5, 2), (0, 5, 3), (1, 4, 1)]),
                        comp(R(9, 23), [(0, 5, 3), (0, 5, 1), (0, 5, 2)]), comp(R(3, 24), [(0, 7, 2)])]
    # two stacked rep0 - 1 before any new offset, over several blocks
    c["rep_stacked"] = [("raw", R(400, 25)), sets, comp(R(9, 26), [(0, 5, 3), (0, 5, 3), (1, 5, 1)]),
                        comp(R(9, 27), [(0, 5, 3), (0, 4, 3), (0, 4, 2)]), comp(b"", [(0, 9, 3)])]
    # rep0 - 1 == 0 that only the incoming offsets show: BAD_BLOCK
    c["rep_zero_incoming"] = [("raw", R(400, 28)), comp(R(9, 29), [(3, 5, 3 + 100), (3, 5, 3 + 1)]),
                              comp(R(9, 30), [(1, 5, 3 + 7), (1, 5, 2)]), comp(R(9, 31), [(0, 5, 3), (1, 5, 3 + 9)]),
                              comp(R(9, 32), [(1, 5, 3 + 20)])]
    # a block without sequences; Raw and RLE blocks between Compressed ones
    c["no_sequences"] = [("raw", R(100, 33)), comp(R(50, 34), []), comp(R(9, 35), [(2, 30, 3 + 120), (0, 9, 1)]),
                         comp(b"", []), comp(R(5, 36), [(0, 5, 1), (0, 30, 3 + 60)])]
    c["raw_rle_between"] = [comp(R(40, 37), [(20, 10, 3 + 10)]), ("raw", R(100, 38)), ("rle", 0x5A, 300),
                            comp(R(10, 39), [(2, 50, 3 + 320), (2, 50, 3 + 100), (0, 5, 2)]), ("rle", 0, 1),
                            comp(R(10, 40), [(1, 20, 3 + 1), (1, 20, 3 + 25), (0, 5, 3)])]
    # more than block_max / 4 sequences in the middle: the block is not marked, which moves the split behind it
    c["dense_middle"] = [("raw", R(100, 41)), comp(R(9, 42), [(2, 9, 3 + 50)]), comp(b"", [(0, 3, 3 + 1)] * 257),
                         comp(R(9, 43), [(2, 9, 3 + 600), (0, 4, 2)]), comp(R(9, 44), [(0, 5, 1), (3, 40, 3 + 800)])]
    return c


@functools.lru_cache(maxsize=None)
def hand(name):
    """-> (frame, content or None where the description cannot be decoded, walk)"""
    blocks = hand_blocks()[name]
    try:
        want = S.content(blocks, block_max=1024)
    except ValueError:
        want = None
    fr = S.frame(blocks, window=WINDOW, fcs=4)
    info = Z.walk(fr)
    assert info["block_max"] == 1024 and 3 <= len(info["blocks"]) <= 6
    return fr, want, info


HAND_NAMES = sorted(hand_blocks())


def one_run(dec, info, lo, hi, hist_bytes, cap=None, damage=None, carry=None):
    """blocks [lo, hi) as one run that goes on, behind `hist_bytes` -> (bytes up to run_len, run_len, status, carry state
    of a good run, par list or None); cap replaces out_cap, damage = (offset, xor mask) into the stream"""
    s, b, r, o = Z.tables(info, lo, hi, hist=len(hist_bytes))
    r = r.copy()
    r["flags"] = int(r["flags"][0]) & ~Z.ZRUN_LAST
    if cap is not None:
        r["out_cap"] = cap
    if damage:
        s = bytearray(s)
        s[damage[0]] ^= damage[1]
        s = bytes(s)
    got = dec(s, b, r, o, history=hist_bytes, carry=carry)
    n, st = int(got[1][0]), int(got[2][0])
    h = len(hist_bytes)
    return (got[0][h:h + n], n, st, P.carry_state(got[3], 0) if st == 0 else P.carry_state(got[3], 0)[4],
            [int(x) for x in got[5]] if len(got) > 5 else None)


def damage_positions(total, count=256, seed=20261018):
    """`count` (offset, bit) pairs spread over a stream of `total` bytes, from a fixed seed"""
    rng = np.random.RandomState(seed)
    return [(int(p), 1 << int(b)) for p, b in zip(rng.randint(0, total, count), rng.randint(0, 8, count))]


def dump_cases(path):
    """the inputs of tools/zstd_par_san.sh: every hand-built frame at every cut (the second call behind the emulated serial
    call's output and carry), and the 256 damaged streams of the damage test -> number of cases"""
    import struct
    recs = []

    def add(s, b, r, o, history=b"", carry=None):
        b, r = np.ascontiguousarray(b, ZSTD_BLOCK), np.ascontiguousarray(r, ZSTD_RUN)
        recs.append(struct.pack("<6I", len(s), len(b), len(r), o, len(history), carry is not None) + bytes(s) + b.tobytes() +
                    r.tobytes() + history + (carry or b""))
    for name in HAND_NAMES:
        info = hand(name)[2]
        n = len(info["blocks"])
        for cut in range(n):
            hist_bytes, cy = b"", None
            for lo, hi in ([(0, n)] if cut == 0 else [(0, cut), (cut, n)]):
                hist = min(len(hist_bytes), info["window"])
                s, b, r, o = Z.tables(info, lo, hi, hist=hist)
                add(s, b, r, o, hist_bytes[len(hist_bytes) - hist:], cy)
                out, rl, st, cy = Z.emu_decode_blocks(s, b, r, o, history=hist_bytes[len(hist_bytes) - hist:], carry=cy)
                if int(st[0]):
                    break
                hist_bytes += out[hist:hist + int(rl[0])]
    for info, nb in ((P.frame(DAMAGE_FRAME)[2], DAMAGE_BLOCKS), (hand("back_1_2_3")[2], 5), (hand("rep_stacked")[2], 5)):
        s, b, r, o = Z.tables(info, 0, nb)
        total = sum(len(x["raw"]) for x in info["blocks"][:nb])
        for pos, bit in damage_positions(total):
            d = bytearray(s)
            d[pos] ^= bit
            add(bytes(d), b, r, o)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    return len(recs)


DAMAGE_FRAME, DAMAGE_BLOCKS = "l19_tiled", 2      # the damage test's input: two blocks, 41 KB of stream, a parallel suffix
