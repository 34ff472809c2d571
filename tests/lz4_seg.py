"""Helpers of the segment-parallel plain .lz4 tests (TEST CODE ONLY): gpumt_lz4_decompress_blocks_seg against
gpumt_lz4_decompress_blocks on block tables, for the emulator and for the device -- lz4_par's cases, hand-built single
blocks whose features sit on segment cuts, failures in a later segment, linked runs of long blocks, liblz4's frames --
and what block_seg has to be, worked out from the tables and the sequence streams alone."""
import ctypes as C

import numpy as np

import emu_driver as E
import helpers as H
import lz4_blocks as B
import lz4_par as P
import lz4_synth as S
from golden import cases
from zstdmt_amd.device import LZ4_BLOCK, LZ4_RUN, LZ4B_STORED

BM, PAD, SENTINEL, TAIL = P.BM, P.PAD, P.SENTINEL, P.TAIL
SEGS = (256, 1024, 65536)


# ---- the new call ------------------------------------------------------------------------------------------------------
def emu_decode(case, seg_bytes, on=1):
    """-> (whole output area, block_len, run_len, status, block_seg)"""
    L = E.lib()
    blocks, runs = np.ascontiguousarray(case["blocks"]), np.ascontiguousarray(case["runs"])
    nblk, nrun, out_bytes = len(blocks), len(runs), case["out_bytes"]
    sbuf = np.frombuffer(bytes(case["stream"]) + b"\xEE" * 8, np.uint8).copy()
    area = np.full(out_bytes + 64, 0xCC, np.uint8)
    area[:len(case["front"])] = np.frombuffer(case["front"], np.uint8)
    bl, bs = np.full(nblk + 1, SENTINEL, np.uint32), np.full(nblk + 1, SENTINEL, np.uint32)
    rl, st = np.full(nrun, 0xA5A5A5A5, np.uint32), np.full(nrun, 99, np.uint32)
    L.emu_lz4_decompress_blocks_seg(E._p(sbuf), C.c_uint64(case.get("stream_bytes", len(case["stream"]))), E._p(blocks),
                                    C.c_uint32(nblk), E._p(runs), C.c_uint32(nrun), E._p(area), C.c_uint64(out_bytes),
                                    E._p(bl), E._p(rl), E._p(st), E._p(bs), C.c_int(on), C.c_uint32(seg_bytes))
    assert int(bl[nblk]) == SENTINEL and int(bs[nblk]) == SENTINEL
    return area, bl[:nblk], rl, st, bs[:nblk]


def gpu_decode(eng, case, seg_bytes):
    assert "stream_bytes" not in case
    prev = eng.set_variant("lz4_seg_bytes", seg_bytes)
    assert prev >= 256
    try:
        out, bl, rl, st, bs = eng.lz4_decompress_blocks_seg(case["stream"], case["blocks"], case["runs"], case["out_bytes"],
                                                            history=case["front"], blk_fill=SENTINEL)
    finally:
        eng.set_variant("lz4_seg_bytes", prev)
    return np.frombuffer(out, np.uint8), bl, rl, st, bs


# ---- what block_seg has to be ------------------------------------------------------------------------------------------
def tokens(body):
    """(input position, output position) of every token of a valid block, then (len(body), decoded length)"""
    def more(n, ip):
        while True:
            v = body[ip]
            ip, n = ip + 1, n + v
            if v != 255:
                return n, ip
    ip, opos, out = 0, 0, []
    while True:
        out.append((ip, opos))
        tok = body[ip]
        lit, ml, ip = tok >> 4, tok & 15, ip + 1
        if lit == 15:
            lit, ip = more(lit, ip)
        ip, opos = ip + lit, opos + lit
        if ip == len(body):
            return out + [(ip, opos)]
        ip += 2
        if ml == 15:
            ml, ip = more(ml, ip)
        opos += ml + 4


def cuts(body, seg):
    """the cuts of a valid block: the first token at or behind k * seg, k = 1, 2, ...; a last token without literals
    starts no segment"""
    tk = tokens(body)
    out, nxt = [], seg
    for ip, opos in tk[:-1]:
        if opos >= nxt:
            out.append((ip, opos))
            nxt = (opos // seg + 1) * seg
    return out[:-1] if out and out[-1][1] == tk[-1][1] else out


def count_segments(body, stored, seg):
    return max(1, -(-len(body) // seg)) if stored else 1 + len(cuts(body, seg))


def expected_block_seg(case, ser, seg):
    """block_seg by the contract of include/gpumt.h: the plan's conditions from the tables, the blocks in front of a run's
    first failing one from the serial call's block_len, their segments from the sequence streams"""
    blocks, runs, ob = case["blocks"], case["runs"], case["out_bytes"]
    nblk = len(blocks)
    want = [0] * nblk
    sb = case.get("stream_bytes", len(case["stream"]))
    hi, owner = 0, [None] * nblk
    for r, R in enumerate(runs):
        first, count, low, off, cap = (int(R[k]) for k in ("first", "count", "low", "out_off", "out_cap"))
        if first > nblk or count > nblk - first or low > off or off > ob or cap > ob - off or off - low > 65536 or not count:
            continue
        if first < hi:
            return want                                   # not ascending and disjoint: the serial code, all of it
        hi = first + count
        for b in range(first, first + count):
            owner[b] = r
    room, total = [0] * nblk, 0
    for b in range(nblk):
        if owner[b] is None:
            continue
        R, K = runs[owner[b]], blocks[b]
        m = int(K["src_len"]) * (1 if int(K["flags"]) & LZ4B_STORED else 255)
        m = min(m, int(K["blkmax"]), 4 << 20, int(R["out_cap"]))
        room[b] = (m - 1) // seg if m else 0
        total += room[b]
        if int(R["count"]) == 1 and not room[b]:
            owner[b] = None
    if total > ob // seg + nblk:
        return want
    for r, R in enumerate(runs):
        first, count = int(R["first"]), int(R["count"])
        if not count or first >= nblk or owner[first] != r:
            continue
        segs = []
        for b in range(first, first + count):
            if int(ser[1][b]) == SENTINEL:
                break
            K = blocks[b]
            body = case["stream"][int(K["src_off"]):int(K["src_off"]) + int(K["src_len"])]
            segs.append(count_segments(body, int(K["flags"]) & LZ4B_STORED, seg))
        if count == 1 and segs == [1]:
            continue                                      # one block of one segment: the serial code
        want[first:first + len(segs)] = segs
    return want


def check(case, ser, new, seg, at_least_two=False):
    """lz4_par.compare, block_seg against expected_block_seg, the case's own `segs` where it states them, and (the
    groups that promise it) two segments or more for every block longer than one"""
    P.compare(case, ser[:4], new[:4])
    got, want = [int(x) for x in new[4]], expected_block_seg(case, ser, seg)
    assert got == want, (case["name"], seg, got, want)
    if "segs" in case and seg in case["segs"]:
        assert got == case["segs"][seg], (case["name"], seg, got)
    elif at_least_two:
        for b, n in enumerate(ser[1]):
            if int(n) != SENTINEL and int(n) > seg:
                assert got[b] >= 2, (case["name"], seg, b, int(n), got[b])


# ---- hand-built blocks -------------------------------------------------------------------------------------------------
class Bld:
    """a sequence list written position by position; `base` = the bytes a match may reach in front of the block"""

    def __init__(self, seed, base=0):
        self.t, self.ti, self.seqs, self.pos, self.base = cases.text(140000, seed), 0, [], 0, base

    def seq(self, nlit, off, ml, check=True):
        assert (not check or 0 < off <= self.base + self.pos + nlit) and self.ti + nlit <= len(self.t)
        self.seqs.append((self.t[self.ti:self.ti + nlit], off, ml))
        self.ti += nlit
        self.pos += nlit + ml
        return self

    def fill_to(self, target):
        """small sequences until fewer than 40 bytes are missing"""
        while self.pos + 40 <= target:
            self.seq(7, min(self.base + self.pos + 7, 33), 20)
        return self

    def land_on(self, target):
        """exactly `target` bytes"""
        self.fill_to(target - 60)
        return self.seq(target - self.pos - 20, 11, 20)

    def cut(self, d):
        """past the next multiple of d: the next token starts a segment at the returned position (for seg_bytes = d)"""
        self.fill_to((self.pos // d + 1) * d)
        self.seq(45, 30, 20)
        assert self.pos % d < 64
        return self.pos

    def end(self, nlit=12):
        self.seqs.append((self.t[self.ti:self.ti + nlit], 0, 0))
        self.pos += nlit
        return ("seq", self.seqs)


def single(name, spec, want=True, segs=None, **kw):
    """one independent block: a run of its own with low = out_off"""
    c = P.one_run(name, [spec], low_at_out=True, **kw)
    c["want"] = [P.expect([spec])] if want else []
    if segs:
        c["segs"] = segs
    return c


def hand_built_single(d):
    """group 2, designed for seg_bytes = d (256 or 1024); every case runs at every seg_bytes of SEGS"""
    out, tag = [], "_d%d" % d
    b = Bld(1).fill_to(d - 50).seq(100, 30, 20).fill_to(3 * d + 10)
    out.append(single("literals_across_a_cut" + tag, b.end()))
    b = Bld(2).fill_to(d - 30).seq(5, 100, 100).fill_to(3 * d + 10)
    out.append(single("match_across_a_cut" + tag, b.end()))
    b = Bld(3)
    b.cut(d)
    b.seq(10, 50, 45).fill_to(b.pos + d)            # source: 40 bytes of the segment before, 5 of this one
    b.cut(d)
    b.seq(3, 60, 60).fill_to(b.pos + 100)
    out.append(single("source_straddles_the_segment_start" + tag, b.end()))
    for o in (1, 3, 7):
        b = Bld(4 + o)
        b.cut(d)
        b.seq(0, o, 50).fill_to(b.pos + d)          # starts in the previous segment's bytes, periodic
        b.cut(d)
        b.seq(2, o, 50 + o).seq(0, 60, 40)          # straddles the start; then its bytes copied again
        b.cut(d)
        b.seq(0, o, 4 * 64 + 9)
        out.append(single("overlap_off%d_from_the_previous_segment" % o + tag, b.end()))
    b = Bld(12)
    starts = [5]
    for k in range(5):                              # every segment starts with the first 30 bytes of the one before
        s = b.cut(d)
        b.seq(0, s - starts[-1], 30)
        starts.append(s)
    b.seq(4, 10, 20)
    out.append(single("chain_of_five_segments" + tag, b.end()))
    b = Bld(13).fill_to(d + 10).seq(5, 40, 3 * d + 500).fill_to(6 * d)
    out.append(single("match_longer_than_three_segments" + tag, b.end()))
    out.append(single("one_match_spans_the_block" + tag, Bld(14).seq(20, 10, 5 * d).end(),
                      segs={s: [2 if 5 * d + 32 > s else 0] for s in SEGS}))
    b = Bld(15).land_on(4 * d - 12)
    spec = b.end()
    assert b.pos == 4 * d
    out.append(single("exactly_four_segments" + tag, spec, segs={d: [4]}))
    b = Bld(16).land_on(2 * d)                      # the last token starts a segment of its own: five literals
    spec = b.end(5)
    out.append(single("last_segment_only_final_literals" + tag, spec, segs={d: [3]}))
    out.append(single("last_token_without_literals" + tag, Bld(17).land_on(2 * d).end(0), want=False))
    out.append(single("stored_several_segments" + tag, ("stored", cases.text(3 * d + 77, 18)), segs={d: [4]}))
    out.append(single("stored_exactly_two_segments" + tag, ("stored", cases.text(2 * d, 19)), segs={d: [2]}))
    b = Bld(20).fill_to(5 * d)
    good = single("block_checksum_good" + tag, b.end(), bcheck=True)
    bad = dict(good, name="block_checksum_bad" + tag, blocks=good["blocks"].copy(), want=[(5, b"")])
    bad["blocks"]["checksum"][0] ^= 1
    return out + [good, bad]


def end_of_block_rules(d=1024):
    """liblz4's end-of-block rules (measured from the block maximum and from the block's last input bytes) where the
    last sequences sit in a late segment: a full 64 KiB block and a short one, final literals 0..5, last match 4..20.
    The verdicts are the serial call's; both must occur"""
    out = []
    for fill, n in ((True, 65536), (False, 3000)):
        for nl in range(6):
            for lm in (4, 8, 14, 15, 20):
                b = Bld(30 + nl).land_on(n - lm - nl - 3).seq(3, 50, lm)
                out.append(single("eob_%s_last%d_m%d" % ("full" if fill else "short", nl, lm), b.end(nl), want=False))
        for back in (11, 12, 13):
            for nl in (1, 5, 7):
                b = Bld(40 + nl).land_on(n - back).seq(0, 8, back - nl)
                out.append(single("eob_%s_back%d_l%d" % ("full" if fill else "short", back, nl), b.end(nl), want=False))
    return out


def failures(d=1024):
    """group 3: what fails sits in a later segment of an independent block"""
    out = []
    b = Bld(50)
    s = b.cut(d)
    b.seq(6, s + 6 + 1, 40, check=False).fill_to(4 * d)   # one byte below the block's first
    c = single("match_below_the_blocks_first_byte", b.end(), want=False)
    c["want"] = [(S.ST_BAD_BLOCK, b"")]
    out.append(c)
    b = Bld(51)
    s = b.cut(d)
    b.seq(6, s + 6, 40).fill_to(4 * d)                    # (the block's first byte itself: accepted)
    out.append(single("match_at_the_blocks_first_byte", b.end()))
    b = Bld(52)
    b.cut(d)
    b.seq(6, 0, 40, check=False).fill_to(4 * d)
    c = single("offset_0", b.end(), want=False)
    c["want"] = [(S.ST_BAD_BLOCK, b"")]
    out.append(c)
    b = Bld(53).fill_to(4 * d)
    spec = b.end()
    body = bytearray(S.block_body(spec[1]))
    tok = S._tokens(spec[1])
    at = tok[next(i for i, (a, _) in enumerate(S._positions(spec[1])) if a >= 2 * d)]
    body[at] = 0xFF                                       # length bytes that run into the literals and past the end
    body[at + 1:at + 4] = b"\xff\xff\xff"
    c = single("malformed_token", ("raw", bytes(body), False), want=False)
    c["want"] = [(S.ST_BAD_BLOCK, b"")]
    out.append(c)
    for cap in (2 * d + 500, 3 * d, 4 * d - 100):
        c = single("out_cap_runs_out_at_%d" % cap, spec, want=False, cap=cap)
        c["want"] = [(S.ST_BAD_BLOCK, b"")]
        out.append(c)
    return out


def linked_runs(d=1024):
    """group 4: three blocks of several segments each behind 64 KiB of history; matches into the block before, across
    two block starts and into the history"""
    hist = cases.text(65536, 60)
    out = []
    for low_at_out in (False, True):
        base = 0 if low_at_out else len(hist)
        spec, done = [], 0
        for k in range(3):
            b = Bld(61 + k, base + done)
            far = min(base + done, 65000)
            b.seq(9, 9 + far if far else 4, 50)                   # as far back as the run may reach
            s = b.cut(d)
            if done:
                b.seq(0, s + 100, 300)                            # from the block before, into this block's segment
                b.seq(5, min(base + done + b.pos, 40000), 64)
            b.fill_to(3 * d + 50 * k)
            s = b.cut(d)
            b.seq(2, min(base + done + s, 65535), 33).fill_to(b.pos + 200)
            spec.append(b.end())
            done += b.pos
        spec.insert(2, ("stored", cases.text(2 * d + 10, 66)))
        c = P.one_run("linked_three_blocks_low_%s" % ("at_out_off" if low_at_out else "below"), spec, hist, low_at_out)
        c["want"] = [P.expect(spec, hist, len(hist) if low_at_out else 0)]
        out.append(c)
    c = P.one_run("linked_three_blocks_bcheck", spec, hist, True, bcheck=True)
    c["want"] = out[1]["want"]
    out.append(c)
    return out


def flip_base(d=1024):
    b = Bld(70)
    s = b.cut(d)
    b.seq(20, s - 100, 40).seq(0, 50, 200).seq(17, 300, 19 + 255 + 3).seq(1, 2, 7).seq(3, s + 10, 9)
    b.cut(d)
    b.seq(3, 700, 40)
    return single("small_independent", b.end()), s


def second_segment_input(case, seg):
    """[first, last) input positions of the case's one block that its second segment reads"""
    c = cuts(case["stream"], seg)
    return c[0][0], c[1][0] if len(c) > 1 else len(case["stream"])


def indep_table(name, bodies, blkmax, data=None, bcheck=False):
    """independent blocks: every one a run of its own with a slot of what it can decode to, as the host engine lays
    them out"""
    import xxhash
    blocks, runs = np.zeros(len(bodies), LZ4_BLOCK), np.zeros(len(bodies), LZ4_RUN)
    stream, at = bytearray(), PAD
    for i, (stored, body) in enumerate(bodies):
        cap = len(body) if stored else min(blkmax, 255 * len(body))
        blocks[i] = (len(stream), len(body), (LZ4B_STORED if stored else 0) | (2 if bcheck else 0), blkmax,
                     xxhash.xxh32(body, seed=0).intdigest() if bcheck else 0)
        runs[i] = (at, at, cap, i, 1, 0)
        stream += body
        at += cap
    c = dict(name=name, stream=bytes(stream), blocks=blocks, runs=runs, out_bytes=at, front=b"\xCC" * PAD)
    if data is not None:
        c["want"] = [(S.ST_OK, data[i * blkmax:(i + 1) * blkmax]) for i in range(len(bodies))]
    return c


def liblz4_cases(n=600 * 1024, block_id=5):
    """group 6: the golden text in frames of independent and of linked 256 KiB blocks"""
    data = cases.text(n, 81)
    out = []
    for linked in (0, 1):
        fr = H.liblz4_frame(data, block_id=block_id, linked=linked, content_size=0, checksum=0)
        info = B.walk(fr)
        bm = info["blkmax"]
        if linked:
            c = P.one_run("liblz4_linked_bd%d" % block_id, [("raw", body, st) for st, body, _ in info["blocks"]], blkmax=bm)
            c["want"] = [(S.ST_OK, data)]
        else:
            c = indep_table("liblz4_independent_bd%d" % block_id, [(st, body) for st, body, _ in info["blocks"]], bm, data)
        out.append(c)
    return out


def dump_cases(path):
    """the tables of groups 2-4 at every seg_bytes for tests/emu/lz4_seg_san.cpp: a count, then per case six words
    (stream bytes, blocks, runs, out bytes, front bytes, seg_bytes), the stream, the two tables and the front"""
    import struct
    todo = [(c, s) for c in hand_built_single(256) + hand_built_single(1024) + linked_runs() for s in SEGS]
    todo += [(c, 1024) for c in failures() + end_of_block_rules()]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(todo)))
        for c, seg in todo:
            blocks, runs = np.ascontiguousarray(c["blocks"]), np.ascontiguousarray(c["runs"])
            f.write(struct.pack("<6I", len(c["stream"]), len(blocks), len(runs), c["out_bytes"], len(c["front"]), seg))
            f.write(c["stream"] + blocks.tobytes() + runs.tobytes() + c["front"])
    return len(todo)
