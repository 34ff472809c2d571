"""Plain .lz4 input decoded block by block (zstdmt_amd/csrc/host/mt_lz4_plain.inc over gpumt_lz4_decompress_blocks and
gpumt_xxh32_carry), on the CPU: the host engine over the emulated device with 16 KiB batches, so a frame spans many
batches, and the new kernels directly under the emulator.  Verdicts are liblz4 1.9.3's wherever it is present."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest
import xxhash

import helpers as H
import lz4_blocks as B
import lz4_synth as S
from golden import cases

HAVE_LIBLZ4 = H.liblz4_frame(b"x") is not None
SEQ = ("seq", [(b"abcdefgh" * 8, 8, 40), (b"tail-literals-xx", 0, 0)])


@pytest.fixture(scope="module")
def lib():
    return B.host_lib()


def decode(lib, st, **kw):
    rv, out, io, stats = H.lz4mt_decompress_via(lib, st, **kw)
    return rv, out, stats


# ---- 1. a frame the parent refuses by its nominal bound ---------------------------------------------------------------
@pytest.mark.parametrize("indep", [True, False])
def test_600_small_blocks_under_block_id_7(lib, indep):
    """600 flushed blocks of 120 bytes under block-size id 7: 54 615 bytes that decode to 72 000, nominal bound 2.4 GB"""
    blocks = [SEQ] * 600
    fr = S.frame(blocks, indep=indep, csize=False, ccheck=True, bd=7)
    want = S.content(blocks, indep)
    assert (len(fr), len(want)) == (54615, 72000)
    ref = S.liblz4_decompress(fr)
    if ref is not None:
        assert ref == (True, want)
    rv, out, stats = decode(lib, fr, threads=2)
    assert rv == 0 and out == want
    assert stats == (0, len(fr), 72000)


# ---- 2. liblz4's own frames, many batches long ------------------------------------------------------------------------
def _content(n, seed):
    return cases.text(n // 2, seed) + cases.rnd(3000, seed + 1) + bytes(9000) + cases.text(n - n // 2, seed + 2)


@pytest.mark.skipif(not HAVE_LIBLZ4, reason="liblz4 not on this box")
@pytest.mark.parametrize("block_id,n", [(4, 200_001), (5, 300_000), (6, 1_100_000), (7, 4_300_000)])
@pytest.mark.parametrize("linked", [1, 0])
@pytest.mark.parametrize("flags", [(0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1)])
def test_liblz4_frames_over_many_batches(lib, block_id, n, linked, flags):
    csize, cchk, bchk = flags
    data = _content(n, block_id * 10 + linked)
    fr = H.liblz4_frame(data, block_id=block_id, linked=linked, content_size=csize, checksum=cchk, block_checksum=bchk)
    assert len(fr) > 5 * 16384          # several batches: the linked carry, the carried checksum, a short last block
    rv, out, stats = decode(lib, fr, threads=3)
    assert rv == 0 and out == data
    assert stats == (0, len(fr), len(data))
    if H.have_ref():
        rv_r, out_r, _, _ = H.lz4mt_decompress_via(H.ref(), fr, threads=3)
        assert rv_r == 0 and out_r == out


# ---- 3. shapes --------------------------------------------------------------------------------------------------------
def _L(n, seed):
    return cases.text(n, seed)


def _many(indep, nblk=40, **kw):
    """a frame of nblk 4 KiB-ish blocks: about ten 16 KiB batches"""
    blocks = []
    for i in range(nblk):
        lits = _L(1500, 100 + i)
        blocks.append(("seq", [(lits, 200 + i, 2500), (b"0123456789ab", 0, 0)]))
    return blocks, S.frame(blocks, indep=indep, **kw)


def _shapes():
    a, b = _L(30000, 5), _L(50000, 6)
    stored_linked = [("seq", [(a[:9000], 100, 400), (a[9000:9012], 0, 0)]), ("stored", b[:40000]),
                     ("seq", [(b"xyz", 40000 + 30, 64), (b"", 80, 64), (a[:12], 0, 0)]), ("stored", b""),
                     ("stored", b[:20000]), ("seq", [(b"q", 20000, 900), (a[:12], 0, 0)])]
    short_mid = [("seq", [(a[:5000], 10, 60000), (a[:12], 0, 0)]), ("seq", [(a[:300], 7, 50), (a[:12], 0, 0)]),
                 ("seq", [(b[:4000], 20, 61000), (a[:12], 0, 0)]), ("stored", b[:777])]
    out = {
        "stored_in_linked": (S.frame(stored_linked, csize=False), S.content(stored_linked)),
        "stored_in_linked_bcheck": (S.frame(stored_linked, bcheck=True), S.content(stored_linked)),
        "short_block_mid_indep": (S.frame(short_mid, indep=True, csize=False), S.content(short_mid, True)),
        "short_block_mid_indep_csize": (S.frame(short_mid, indep=True, bd=6), S.content(short_mid, True)),
        "empty": (S.frame([], csize=False), b""),
        "empty_csize_nocheck": (S.frame([], ccheck=False), b""),
        "dictid": (S.frame(short_mid, indep=True, dict_id=77), S.content(short_mid, True)),
    }
    f1, c1 = out["stored_in_linked"]
    f2, c2 = out["short_block_mid_indep"]
    skip = struct.pack("<II", 0x184D2A53, 70000) + bytes(70000)      # a skippable frame longer than several batches
    out["frames_and_skippables"] = (f1 + skip + out["empty"][0] + f2 + struct.pack("<II", 0x184D2A50, 0) + f1,
                                    c1 + c2 + c1)
    # a linked frame that ends in the batch in which the next one starts (its carry is used behind a new frame header)
    lb, lf = _many(False, nblk=23, csize=False)
    ib, jf = _many(True, nblk=9)
    out["linked_frames_back_to_back"] = (lf + lf + jf + lf, S.content(lb) * 2 + S.content(ib, True) + S.content(lb))
    recs = H.oracle_compress(a, 4096)
    out["frame_then_records"] = (f2 + recs, c2 + a)
    return out


@pytest.mark.parametrize("kind", ["empty", "one_block_indep", "one_block_linked"])
def test_more_frames_than_a_batch_has_table_entries(lib, kind):
    """more than 8192 frames inside one batch of input (a file of one frame per message): the batch's tables fill up in
    front of a frame header, which the next batch reads again"""
    if kind == "empty":
        fr, want, n = S.frame([], csize=False, ccheck=False), b"", 8192 * 2 + 5          # 11 bytes each: 1489 per batch
        assert len(fr) * 8193 < 16384 * 8
    else:
        blocks = [("seq", [(b"0123456789abcdefghij", 7, 30), (b"0123456789ab", 0, 0)])]
        fr, want, n = S.frame(blocks, indep=kind.endswith("indep")), S.content(blocks), 8192 + 700
    st = fr * n
    env = dict(os.environ, GPUMT_BATCH_KB="2048")
    code = ("import sys; sys.path[:0] = %r; import helpers as H, lz4_blocks as B, hashlib; L = B.host_lib(2048); "
            "rv, out, _, stats = H.lz4mt_decompress_via(L, open(sys.argv[1], 'rb').read(), threads=2); "
            "print(rv, len(out), hashlib.sha256(out).hexdigest(), stats[1])" % (sys.path[:4],))
    import hashlib
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".lz4") as f:       # a process of its own: the batch size is read once
        f.write(st)
        f.flush()
        p = subprocess.run([sys.executable, "-c", code, f.name], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-800:]
    assert p.stdout.split() == ["0", str(len(want) * n), hashlib.sha256(want * n).hexdigest(), str(len(st))]
    if kind == "empty":                                         # and with the 16 KiB batches of this module
        rv, out, stats = decode(lib, st)
        assert rv == 0 and out == b"" and stats == (0, len(st), 0)


@pytest.mark.parametrize("name", sorted(_shapes()))
def test_shapes(lib, name):
    st, want = _shapes()[name]
    rv, out, stats = decode(lib, st, threads=2)
    assert rv == 0 and out == want
    assert stats == (0, len(st), len(want))
    if name in ("stored_in_linked", "short_block_mid_indep", "empty", "dictid") and S.liblz4_path():
        assert S.liblz4_decompress(st) == (True, want)


# ---- 4. rejections, each against liblz4 -------------------------------------------------------------------------------
def _rejections():
    out = {}
    for indep in (True, False):
        tag = "indep" if indep else "linked"
        blocks, fr = _many(indep, csize=False)
        good = S.content(blocks, indep)
        out["ok_" + tag] = (fr, good)
        bad = bytearray(fr)
        bad[6] ^= 0x10                                  # header checksum byte
        out["header_checksum_" + tag] = (bytes(bad), None)
        bad = bytearray(fr)
        bad[-1] ^= 0x04                                 # content checksum, checked with the last batch
        out["content_checksum_last_batch_" + tag] = (bytes(bad), None)
        out["wrong_content_size_" + tag] = (S.frame(blocks, indep=indep, content_size=len(good) + 1), None)
        out["right_content_size_" + tag] = (S.frame(blocks, indep=indep), good)
        _, frb = _many(indep, csize=False, bcheck=True)
        out["ok_bcheck_" + tag] = (frb, good)
        bad = bytearray(frb)
        bad[len(frb) // 2] ^= 0x01                      # inside a block of a middle batch: its checksum no longer fits
        out["block_checksum_middle_batch_" + tag] = (bytes(bad), None)
    big = ("raw", S.block_body([(_L(65537 - 9, 3), 0, 0)]), False)
    out["block_above_max"] = (S.frame([SEQ, big], csize=False, ccheck=False), None)
    out["stored_above_max"] = (S.frame([SEQ, ("raw", _L(65537, 4), True)], csize=False, ccheck=False), None)
    # linked offsets: 65535 back over two stored blocks is fine, one byte before the frame start is not, and in an
    # independent frame nothing before the block is
    s64 = _L(65536, 7)
    far = [("stored", s64[:30000]), ("stored", s64[:35600]), ("seq", [(b"abc", 65535, 40), (b"0123456789ab", 0, 0)])]
    out["ok_offset_65535_linked"] = (S.frame(far, csize=False), S.content(far))
    near = [("stored", s64[:3000]), ("seq", [(b"abc", 3004, 40), (b"0123456789ab", 0, 0)])]
    out["offset_before_frame_start"] = (S.frame(near, csize=False), None)
    out["ok_offset_at_frame_start"] = (S.frame([near[0], ("seq", [(b"abc", 3003, 40), (b"0123456789ab", 0, 0)])],
                                               csize=False), None)
    out["ok_offset_at_frame_start"] = (out["ok_offset_at_frame_start"][0],
                                       S.content([near[0], ("seq", [(b"abc", 3003, 40), (b"0123456789ab", 0, 0)])]))
    out["offset_across_indep_blocks"] = (S.frame(near, csize=False, indep=True), None)
    many_far = [("stored", s64[:20000])] * 5 + [("seq", [(b"abc", 65535, 40), (b"0123456789ab", 0, 0)])]
    out["ok_offset_65535_over_batches"] = (S.frame(many_far, csize=False), S.content(many_far))
    out["trailing_garbage"] = (out["ok_linked"][0] + b"garbage!", None)
    return out


@pytest.mark.parametrize("name", sorted(_rejections()))
def test_verdicts_match_liblz4(lib, name):
    st, want = _rejections()[name]
    ref = S.liblz4_decompress(st)
    if ref is not None:
        assert ref[0] == (want is not None), "the case is not what liblz4 says it is"
        if want is not None:
            assert ref[1] == want
    rv, out, stats = decode(lib, st, threads=2)
    if want is None:
        assert rv == B.ERR(B.E_LIB), (rv, lib.LZ4MT_getErrorString(rv))
    else:
        assert rv == 0 and out == want and stats == (0, len(st), len(want))


def test_truncation_at_every_state_of_the_walker(lib):
    """cut inside the header, a block header, a block body, a block checksum, the end mark, the content checksum, a
    skippable frame's header and body: always an error, and what was written before is a prefix"""
    blocks, fr = _many(False, nblk=12, bcheck=True)
    info = B.walk(fr)
    good = S.content(blocks)
    body0 = 7 + 4                                            # first block body starts here
    b0 = len(info["blocks"][0][1])
    cuts = [5, 6, 7, 9, body0 + 10, body0 + b0, body0 + b0 + 2, body0 + b0 + 4 + 2, len(fr) // 2,
            len(fr) - 9, len(fr) - 8, len(fr) - 6, len(fr) - 4, len(fr) - 3, len(fr) - 1]
    for cut in cuts:
        rv, out, _ = decode(lib, fr[:cut])
        assert rv == B.ERR(B.E_LIB), cut
        assert good.startswith(out), cut
        if S.liblz4_path():
            assert S.liblz4_decompress(fr[:cut])[0] is False
    skip = struct.pack("<II", 0x184D2A51, 100) + bytes(100)
    for cut in (len(fr) + 3, len(fr) + 6, len(fr) + 8, len(fr) + 50):
        rv, out, _ = decode(lib, (fr + skip)[:cut])
        assert rv == B.ERR(B.E_LIB) and out == good, cut
    rv, out, _ = decode(lib, fr + skip)
    assert rv == 0 and out == good


# ---- 5. host memory ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indep", [True, False])
def test_reads_stay_about_two_batches_ahead_of_the_writes(lib, indep):
    """a frame some forty batches long: when a piece is written, the bytes read so far are at most two batches and one
    block (plus a request) past the input that piece came from"""
    batch, request = 16384, 4096
    blocks, fr = _many(indep, nblk=400, csize=False)
    good = S.content(blocks, indep)
    info = B.walk(fr)
    ends, at, pos = [], 0, 7              # (content offset, input offset) where each block ends
    for (stored, body, _), b in zip(info["blocks"], blocks):
        pos += 4 + len(body)
        at += len(S.content([b], True))
        ends.append((at, pos))
    assert len(fr) > 30 * batch
    io = H.MemIO(fr)
    ahead = []

    def write(_arg, bufp):
        done = sum(io.writes) + bufp.contents.size
        consumed = next(p for a, p in ends if a >= done)
        ahead.append(io.pos - consumed)
        return H.MemIO._write(io, _arg, bufp)
    wr = H.RD_FN(write)
    io.rdwr = H.RefRdWr(io._rd, None, wr, None)
    ctx = lib.LZ4MT_createDCtx(2, request)
    rv = lib.LZ4MT_decompressDCtx(ctx, C.byref(io.rdwr))
    lib.LZ4MT_freeDCtx(ctx)
    assert rv == 0 and io.result() == good
    assert len(io.writes) > 30
    biggest = max(len(b[1]) for b in info["blocks"]) + 8
    assert max(ahead) <= 2 * batch + biggest + request, max(ahead)
    assert io.reads[0][0] == 4 and all(w == request for w, _ in io.reads[1:])    # the sniff, then the context's request size


# ---- 6. the kernels directly ------------------------------------------------------------------------------------------
def _kernel_cases():
    man = __import__("test_emu_lz4_synth").MAN
    fam = S.families(man["seed"])
    return man, fam


def test_block_kernel_on_the_synth_families():
    """every family re-framed as a block table: liblz4's verdict (the manifest) and content; rejected cases report
    BAD_BLOCK on the run and accepted ones decode with every slot's length right"""
    man, fam = _kernel_cases()
    bad = []
    for name in sorted(fam):
        e, m = fam[name], man["cases"][name]
        info = B.walk(e["frame"])
        if not info["blocks"]:
            continue
        stream, blocks, runs, out_bytes = B.tables(info)
        out, bl, rl, st = B.emu_decode_blocks(stream, blocks, runs, out_bytes, pack=True)
        accept = m["liblz4"] == "accept"
        if name in ("bad_short_of_csize", "bad_past_csize"):      # the size field is the host's to check
            accept = True
        if name in ("bad_block_above_max", "bad_stored_above_max"):
            assert list(st) == [S.ST_BAD_BLOCK], name
            continue
        if accept:
            want = e["content"]
            if list(st) != [0] * len(st) or out != want or int(bl.sum()) != len(want):
                bad.append((name, list(st), len(out), len(want)))
        elif S.ST_BAD_BLOCK not in st or not all(int(x) in (0, S.ST_BAD_BLOCK) for x in st):
            bad.append((name, list(st)))          # rejected: at least one run BAD_BLOCK, none anything else
    assert not bad, bad


def test_block_kernel_history_and_table_checks():
    data = cases.text(200000, 9)
    if HAVE_LIBLZ4:
        fr = H.liblz4_frame(data, block_id=4, linked=1)
        info = B.walk(fr)
        # the second half of the blocks as a run of its own behind 64 KiB of history
        k = len(info["blocks"]) // 2
        head = dict(info, blocks=info["blocks"][:k])
        tail = dict(info, blocks=info["blocks"][k:])
        s1, b1, r1, o1 = B.tables(head)
        out1, _, rl1, st1 = B.emu_decode_blocks(s1, b1, r1, o1)
        assert list(st1) == [0] and out1[:int(rl1[0])] == data[:int(rl1[0])]
        hist = data[int(rl1[0]) - 65536:int(rl1[0])]
        s2, b2, r2, o2 = B.tables(tail, history=65536)
        out2, _, rl2, st2 = B.emu_decode_blocks(s2, b2, r2, o2, history=hist)
        assert list(st2) == [0] and out2[65536:65536 + int(rl2[0])] == data[int(rl1[0]):]
        # without the history the same run must not read in front of its output
        r2n = r2.copy()
        r2n["low"] = r2n["out_off"]
        _, _, _, st3 = B.emu_decode_blocks(s2, b2, r2n, o2, history=hist)
        assert list(st3) == [S.ST_BAD_BLOCK]
    # table entries that leave the stream or the output are refused, nothing is written
    info = B.walk(S.frame([SEQ, SEQ], indep=True))
    s, b, r, o = B.tables(info)
    for field, val, arr in (("src_off", len(s) + 1, "b"), ("src_len", len(s) + 1, "b"), ("out_off", o + 1, "r"),
                            ("out_cap", o + 1, "r"), ("first", 3, "r"), ("count", 3, "r"), ("blkmax", 100, "b")):
        bb, rr = b.copy(), r.copy()
        (bb if arr == "b" else rr)[field][0] = val
        if field == "out_off":
            rr["low"][0] = val
        out, _, rl, st = B.emu_decode_blocks(s, bb, rr, o)
        assert int(st[0]) == 1 and int(rl[0]) == 0 and int(st[1]) == 0, field
    rr = r.copy()
    rr["low"][1] = 0
    rr["out_off"][1] = 70000
    out, _, rl, st = B.emu_decode_blocks(s, b, rr, 80000)
    assert int(st[1]) == 1                                          # more than 64 KiB of history


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 100, 4096, 70001])
def test_xxh32_carried_state(n):
    data = cases.rnd(n, n + 3)
    want = xxhash.xxh32(data, seed=0).intdigest()
    splits = [[n], [0, n], [n, 0], [n // 2, n - n // 2], [min(n, 3), max(n - 3, 0)], [min(n, 16), max(n - 16, 0)]]
    if n >= 40:
        splits += [[5, 7, 4, 16, n - 32], [1] * 20 + [n - 20], [15, 1, 17, n - 33]]
    for pieces in splits:
        assert B.emu_xxh32_carry(data, pieces) == want, pieces


def test_new_kernels_under_the_strict_emulator():
    env = dict(os.environ, EMU_STRICT="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "block_kernel or xxh32_carried"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-1500:]
