"""Helpers of the block-parallel linked-run tests (TEST CODE ONLY): one list of block tables -- hand-built streams, linked
frames written by liblz4 and cut at every block boundary, damaged input -- and the comparison of
gpumt_lz4_decompress_blocks_par with gpumt_lz4_decompress_blocks on each, for the emulator and for the device."""
import ctypes as C

import numpy as np

import emu_driver as E
import helpers as H
import lz4_blocks as B
import lz4_synth as S
from golden import cases
from zstdmt_amd.device import LZ4_BLOCK, LZ4_RUN, LZ4B_STORED, LZ4B_CHECKSUM

BM = 65536
PAD = 32            # guard bytes in front of the history
SENTINEL = 0x5E5E5E5E
TAIL = b"0123456789ab"
HAVE_LIBLZ4 = H.liblz4_frame(b"x") is not None


# ---- the two calls under the emulator ---------------------------------------------------------------------------------
def emu_decode(case, par):
    """-> (whole output area, block_len, run_len, status)"""
    L = E.lib()
    blocks, runs = np.ascontiguousarray(case["blocks"]), np.ascontiguousarray(case["runs"])
    nblk, nrun, out_bytes = len(blocks), len(runs), case["out_bytes"]
    sbuf = np.frombuffer(bytes(case["stream"]) + b"\xEE" * 8, np.uint8).copy()
    area = np.full(out_bytes + 64, 0xCC, np.uint8)
    area[:len(case["front"])] = np.frombuffer(case["front"], np.uint8)
    bl = np.full(nblk + 1, SENTINEL, np.uint32)
    rl, st = np.full(nrun, 0xA5A5A5A5, np.uint32), np.full(nrun, 99, np.uint32)
    args = [E._p(sbuf), C.c_uint64(case.get("stream_bytes", len(case["stream"]))), E._p(blocks), C.c_uint32(nblk),
            E._p(runs), C.c_uint32(nrun), E._p(area), C.c_uint64(out_bytes), E._p(bl), E._p(rl), E._p(st)]
    if par:
        L.emu_lz4_decompress_blocks_par(*args, C.c_int(1))
    else:
        L.emu_lz4_decompress_blocks(*args)
    assert int(bl[nblk]) == SENTINEL
    return area, bl[:nblk], rl, st


def gpu_decode(eng, case, par):
    f = eng.lz4_decompress_blocks_par if par else eng.lz4_decompress_blocks
    assert "stream_bytes" not in case
    out, bl, rl, st = f(case["stream"], case["blocks"], case["runs"], case["out_bytes"], history=case["front"],
                        blk_fill=SENTINEL)
    return np.frombuffer(out, np.uint8), bl, rl, st


def compare(case, ser, par):
    """the new call against the serial one: bytes over [out_off, out_off + run_len), the whole block_len array, run_len,
    status, and every byte outside the runs' areas; `want` (per run: status, content or None) pins the case itself"""
    (oa, bla, rla, sta), (ob, blb, rlb, stb) = ser, par
    name = case["name"]
    assert list(stb) == list(sta), (name, list(sta), list(stb))
    assert list(rlb) == list(rla), (name, list(rla), list(rlb))
    assert list(blb) == list(bla), (name, list(bla), list(blb))
    keep = np.ones(case["out_bytes"], bool)
    for r, R in enumerate(case["runs"]):
        a, n, cap = int(R["out_off"]), int(rla[r]), int(R["out_cap"])
        if a + cap <= case["out_bytes"]:
            keep[a:a + cap] = False
            assert bytes(ob[a:a + n]) == bytes(oa[a:a + n]), (name, r)
    init = np.full(case["out_bytes"], 0xCC, np.uint8)
    init[:len(case["front"])] = np.frombuffer(case["front"], np.uint8)
    for o in (oa, ob):
        assert (o[:case["out_bytes"]][keep] == init[keep]).all(), (name, "a byte outside the runs' areas changed")
    for r, (wst, wdata) in enumerate(case.get("want", [])):
        assert int(sta[r]) == wst, (name, r, int(sta[r]), wst)
        if wdata is not None:
            a = int(case["runs"][r]["out_off"])
            assert int(rla[r]) == len(wdata) and bytes(oa[a:a + len(wdata)]) == wdata, (name, r, "content")


# ---- tables -----------------------------------------------------------------------------------------------------------
def one_run(name, spec, hist=b"", low_at_out=False, cap=None, blkmax=BM, bcheck=False):
    """the blocks of `spec` -- ("seq", seqs) / ("stored", bytes) / ("raw", body, stored) -- as one run behind `hist`"""
    import xxhash
    blocks = np.zeros(len(spec), LZ4_BLOCK)
    stream, room = bytearray(), 0
    for i, b in enumerate(spec):
        body, stored = (b[1], True) if b[0] == "stored" else (S.block_body(b[1]), False) if b[0] == "seq" else (b[1], b[2])
        blocks[i] = (len(stream), len(body), (LZ4B_STORED if stored else 0) | (LZ4B_CHECKSUM if bcheck else 0), blkmax,
                     xxhash.xxh32(body, seed=0).intdigest() if bcheck else 0)
        stream += body
        room += len(body) if stored else min(blkmax, 255 * len(body))
    runs = np.zeros(1, LZ4_RUN)
    out_off = PAD + len(hist)
    cap = room if cap is None else cap
    runs[0] = (out_off if low_at_out else PAD, out_off, cap, 0, len(spec), 0)
    return dict(name=name, stream=bytes(stream), blocks=blocks, runs=runs, out_bytes=out_off + cap,
                front=b"\xCC" * PAD + hist)


def expect(spec, hist=b"", low=0):
    """what the blocks decode to behind hist (matches may reach hist[low]) -> (status, content before the first bad block)"""
    out, done = bytearray(hist), len(hist)
    for b in spec:
        try:
            if b[0] == "stored":
                out += b[1]
            else:
                S.decode_seqs(b[1], out, low)
        except ValueError:
            return S.ST_BAD_BLOCK, bytes(out[len(hist):done])
        done = len(out)
    return S.ST_OK, bytes(out[len(hist):])


def hand_built():
    t = cases.text(70000, 21)
    out = []

    def add(name, spec, hist=b"", low_at_out=False, **kw):
        c = one_run(name, spec, hist, low_at_out, **kw)
        c["want"] = [expect(spec, hist, len(hist) if low_at_out else 0)]
        out.append(c)
    # a match at distance exactly 65535 into block 0, a source that starts 7 bytes before block 1 and runs into it with
    # off < ml, and a match inside block 1 that copies those bytes again (overlapping as well)
    b1 = ("seq", [(b"abc", 65535, 40), (b"", 50, 200), (b"", 100, 150), (b"xy", 393, 30), (TAIL, 0, 0)])
    add("dist_65535_straddle_recopy", [("stored", t[:65536]), b1])
    add("dist_65535_in_block_2", [("stored", t[:65436]), ("seq", [(t[:20], 7, 68), (TAIL, 0, 0)]), b1])
    # block 2 copies bytes of block 1 that block 1 copied from block 0; block 1 has 100 bytes, so the next origin
    # crosses two block starts
    chain = [("stored", t[:5000]), ("seq", [(t[100:110], 4000, 78), (TAIL, 0, 0)]),
             ("seq", [(b"Q", 60, 50), (b"", 51 + 100 + 2000, 300), (b"", 351 + 100 + 5000, 9), (TAIL, 0, 0)])]
    add("three_block_chain", chain)
    add("three_block_chain_bcheck", chain, bcheck=True)
    add("stored_in_the_middle", [("seq", [(t[:9000], 100, 400), (TAIL, 0, 0)]), ("stored", t[20000:60000]),
                                 ("seq", [(b"xyz", 40000 + 30, 64), (b"", 80, 64), (TAIL, 0, 0)]), ("stored", b""),
                                 ("stored", t[:200]), ("seq", [(b"q", 250, 900), (TAIL, 0, 0)])])
    # history below out_off: read by block 0, by block 1 across block 0, with low < out_off and with low == out_off
    hist = t[30000:33000]
    reach0 = [("seq", [(b"abc", 2000, 40), (TAIL, 0, 0)]), ("seq", [(b"de", 57 + 1500, 70), (b"", 30, 33), (TAIL, 0, 0)])]
    reach1 = [("seq", [(t[:50], 20, 40), (TAIL, 0, 0)]), reach0[1], ("stored", t[:300])]
    for nm, spec in (("history_block0", reach0), ("history_block1", reach1)):
        add(nm + "_low_below", spec, hist)
        add(nm + "_low_at_out_off", spec, hist, low_at_out=True)
    add("one_block", [b1], hist=t[:65536])
    add("one_block_no_history", [("seq", [(t[:50], 20, 40), (TAIL, 0, 0)])])
    # an offset one byte beyond low, in block 0 and in block 2 (and the last one that is still inside)
    for d, tag in ((1, "beyond"), (0, "at")):
        add("offset_%s_low_block0" % tag, [("seq", [(b"abc", 3003 + d, 40), (TAIL, 0, 0)]), reach1[0], reach1[0]], hist)
        add("offset_%s_low_block2" % tag,
            [reach1[0], ("stored", t[:700]), ("seq", [(b"abc", 3000 + 102 + 700 + 3 + d, 40), (TAIL, 0, 0)]), reach1[0]], hist)
    # no room: the third block does not fit the capacity, by one byte and by a whole block
    fit = [("stored", t[:1000]), reach1[0], ("seq", [(t[:40], 1100, 500), (TAIL, 0, 0)]), ("stored", t[:10])]
    lens = [1000, 102, 552, 10]
    for short in (0, 10, 11, 300, 600):
        c = one_run("room_short_by_%d" % short, fit, cap=sum(lens) - short)
        nfit = max(k for k in range(5) if sum(lens[:k]) <= sum(lens) - short)
        c["want"] = [(S.ST_OK if nfit == 4 else S.ST_BAD_BLOCK, expect(fit[:nfit])[1])]
        out.append(c)
    return out


def cut_frames():
    """linked frames of liblz4 over text, a period-300 pattern, zeros and random bytes, 64 KiB and 256 KiB blocks, as two
    batches cut at every block boundary: the second one decodes behind the last 64 KiB of the first one's content"""
    out = []
    if not HAVE_LIBLZ4:
        return out
    pat = (cases.rnd(300, 8) * 2000)
    for block_id, n in ((4, 65536 * 3 + 30001), (5, 262144 * 2 + 50001)):
        kinds = dict(text=cases.text(n, 31 + block_id), period300=pat[:n], zeros=bytes(n),
                     random=cases.rnd(n // 2, 5) + cases.text(n - n // 2, 6))
        for kind, data in sorted(kinds.items()):
            fr = H.liblz4_frame(data, block_id=block_id, linked=1, content_size=0, checksum=0,
                                block_checksum=1 if kind == "text" else 0)
            info = B.walk(fr)
            bm, nb = info["blkmax"], len(info["blocks"])
            assert nb >= 3
            for k in list(range(1, nb)) + [nb]:
                for part, (lo, hi) in enumerate(((0, k), (k, nb))):
                    if lo == hi:
                        continue
                    spec = [("raw", body, stored) for stored, body, _ in info["blocks"][lo:hi]]
                    hist = data[max(0, lo * bm - 65536):lo * bm]
                    c = one_run("liblz4_%s_bd%d_cut%d_part%d" % (kind, block_id, k, part), spec, hist, blkmax=bm,
                                bcheck=info["bchk"])
                    c["want"] = [(S.ST_OK, data[lo * bm:hi * bm])]
                    out.append(c)
    return out


def tables_of_many_runs():
    """two linked runs and single blocks in one table; the same with the runs in descending block order, which the plan
    refuses (everything decodes serially); a run that names blocks of another one"""
    t = cases.text(20000, 77)
    a = [("stored", t[:3000]), ("seq", [(t[:50], 2000, 400), (TAIL, 0, 0)]), ("seq", [(b"ab", 3300, 40), (TAIL, 0, 0)])]
    b = [("seq", [(t[500:900], 100, 300), (TAIL, 0, 0)]), ("seq", [(b"", 700, 712), (TAIL, 0, 0)])]
    single = [("seq", [(t[:50], 20, 40), (TAIL, 0, 0)])]
    parts = [one_run("p", s) for s in (a, single, b, single)]
    want = [expect(s) for s in (a, single, b, single)]

    def join(name, order, extra=None):
        nblk = sum(len(p["blocks"]) for p in parts)
        blocks, runs = np.zeros(nblk, LZ4_BLOCK), np.zeros(len(parts) + (1 if extra else 0), LZ4_RUN)
        stream, at, bi, where = bytearray(), PAD, 0, {}
        for i, p in enumerate(parts):
            blk = p["blocks"].copy()
            blk["src_off"] += len(stream)
            blocks[bi:bi + len(blk)] = blk
            cap = int(p["runs"][0]["out_cap"])
            where[i] = (at, at, cap, bi, len(blk), 0)
            stream += p["stream"]
            bi += len(blk)
            at += cap + 16
        for slot, i in enumerate(order):
            runs[slot] = where[i]
        w = [want[i] for i in order]
        if extra:                      # one more run over blocks 1..2 of the first run, with an area of its own
            runs[len(parts)] = (at, at, 70000, 1, 2, 0)
            w.append((S.ST_BAD_BLOCK, b""))
            at += 70000
        return dict(name=name, stream=bytes(stream), blocks=blocks, runs=runs, out_bytes=at, front=b"\xCC" * PAD, want=w)
    return [join("many_runs_ascending", [0, 1, 2, 3]), join("many_runs_descending", [2, 3, 0, 1]),
            join("many_runs_overlapping", [0, 1, 2, 3], extra=True)]


def damaged_tables():
    t = cases.text(66000, 41)
    spec = [("stored", t[:2000]), ("seq", [(t[:30], 1500, 40), (b"", 50, 200), (t[:16], 0, 0)]),
            ("seq", [(b"abc", 2200, 40), (TAIL, 0, 0)])]
    out = []
    c = one_run("block_checksum_1_of_3", spec, bcheck=True)
    c["blocks"]["checksum"][1] ^= 0x100
    c["want"] = [(5, t[:2000])]
    out.append(c)
    c = one_run("src_len_above_blkmax", [spec[0], ("stored", t[:65537]), spec[2]])
    c["want"] = [(S.ST_BAD_BLOCK, t[:2000])]
    out.append(c)
    c = one_run("entry_leaves_the_stream", spec)
    c["blocks"]["src_off"][1] = len(c["stream"]) - 3
    c["want"] = [(1, t[:2000])]
    out.append(c)
    c = one_run("entry_leaves_the_stream_last_block", spec)
    c["stream_bytes"] = len(c["stream"]) - 1      # (emulator only: the device wrapper passes the stream's own size)
    c["want"] = [(1, expect(spec[:2])[1])]
    out.append(c)
    c = one_run("blkmax_below_64k", spec)
    c["blocks"]["blkmax"][2] = 4096
    c["want"] = [(1, expect(spec[:2])[1])]
    out.append(c)
    return out


def flips(case, block, positions, masks=(0xFF,)):
    """`case` with one byte of block `block` changed, per position and mask"""
    at, n = int(case["blocks"]["src_off"][block]), int(case["blocks"]["src_len"][block])
    for p in positions:
        for m in masks:
            st = bytearray(case["stream"])
            st[at + p % n] ^= m
            yield dict(case, name="%s_flip%d_%02x" % (case["name"], p % n, m), stream=bytes(st), want=[])


def flip_base_small():
    """a small linked run whose second block holds literals, far and near matches, a straddling one and length bytes"""
    t = cases.text(5000, 43)
    spec = [("stored", t[:3000]),
            ("seq", [(t[:20], 2500, 40), (b"", 50, 200), (t[100:117], 300, 19 + 255 + 3), (b"z", 2, 7), (t[:13], 0, 0)]),
            ("seq", [(b"abc", 3400, 40), (b"", 45, 20), (TAIL, 0, 0)])]
    c = one_run("small_linked", spec)
    c["want"] = [expect(spec)]
    return c


def flip_base_liblz4():
    data = cases.text(65536 * 2 + 9000, 47)
    info = B.walk(H.liblz4_frame(data, block_id=4, linked=1, content_size=0, checksum=0))
    c = one_run("liblz4_text", [("raw", body, stored) for stored, body, _ in info["blocks"]])
    c["want"] = [(S.ST_OK, data)]
    return c


def all_cases(device=False):
    out = hand_built() + cut_frames() + tables_of_many_runs() + damaged_tables()
    return [c for c in out if not (device and "stream_bytes" in c)]
