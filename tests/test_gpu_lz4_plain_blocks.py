"""Plain .lz4 input decoded block by block, on the device: the families of tests/test_emu_lz4_plain_blocks.py through
LZ4MT_decompressDCtx and the command line tools, gpumt_lz4_decompress_blocks / gpumt_xxh32_carry directly, and one
frame whose content is above 2 GiB."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest
import xxhash

import helpers as H
import lz4_blocks as B
import lz4_synth as S
import test_emu_lz4_plain_blocks as T
from golden import cases

pytestmark = pytest.mark.gpu

BIN = os.path.join(H.ROOT, "zstdmt_amd", "bin")


@pytest.fixture(scope="module")
def lib():
    from zstdmt_amd._native import lib_path
    return H.bind_lz4mt(C.CDLL(lib_path()))


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


# ---- 7. the families through the API and the kernels directly ---------------------------------------------------------
@pytest.mark.parametrize("indep", [True, False])
def test_600_small_blocks_under_block_id_7(lib, indep):
    blocks = [T.SEQ] * 600
    fr = S.frame(blocks, indep=indep, csize=False, ccheck=True, bd=7)
    rv, out, _, stats = H.lz4mt_decompress_via(lib, fr, threads=2)
    assert rv == 0 and out == S.content(blocks, indep)
    assert stats == (0, len(fr), 72000)


@pytest.mark.parametrize("name", sorted(T._shapes()))
def test_shapes(lib, name):
    st, want = T._shapes()[name]
    rv, out, _, stats = H.lz4mt_decompress_via(lib, st, threads=2)
    assert rv == 0 and out == want
    assert stats == (0, len(st), len(want))


@pytest.mark.parametrize("name", sorted(T._rejections()))
def test_verdicts_match_liblz4(lib, name):
    st, want = T._rejections()[name]
    ref = S.liblz4_decompress(st)
    if ref is not None:
        assert ref[0] == (want is not None)
    rv, out, _, stats = H.lz4mt_decompress_via(lib, st, threads=2)
    if want is None:
        assert rv == B.ERR(B.E_LIB), rv
    else:
        assert rv == 0 and out == want and stats == (0, len(st), len(want))


@pytest.mark.skipif(not T.HAVE_LIBLZ4, reason="liblz4 not on this box")
@pytest.mark.parametrize("block_id", [4, 5, 6, 7])
@pytest.mark.parametrize("linked", [1, 0])
def test_liblz4_frames_over_many_batches(block_id, linked):
    """16 MiB batches (a process of its own: the batch size is read once), 70 MiB of content per frame; content size,
    content checksum and block checksums in turn"""
    data = cases.text(70 << 20, seed=block_id) + cases.rnd(1 << 20, 3)
    k = block_id + linked
    fr = H.liblz4_frame(data, block_id=block_id, linked=linked, content_size=k & 1, checksum=(k >> 1) & 1,
                        block_checksum=1 if block_id == 5 else 0)
    env = dict(os.environ, GPUMT_BATCH_MB="16", GPUMT_TRACE="1")
    r = subprocess.run([os.path.join(BIN, "lz4cat-mt")], input=fr, capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-300:]
    assert r.stdout == data
    assert b"[lz4mt plain]" in r.stderr and b" 1 batches" not in r.stderr


def test_block_kernel_on_the_synth_families(eng):
    """Engine.lz4_decompress_blocks against liblz4's verdicts (the manifest) and the builder's content"""
    man, fam = T._kernel_cases()
    bad = []
    for name in sorted(fam):
        e, m = fam[name], man["cases"][name]
        info = B.walk(e["frame"])
        if not info["blocks"]:
            continue
        stream, blocks, runs, out_bytes = B.tables(info)
        out, bl, rl, st = eng.lz4_decompress_blocks(stream, blocks, runs, out_bytes, pack=True)
        out_e, bl_e, rl_e, st_e = B.emu_decode_blocks(stream, blocks, runs, out_bytes, pack=True)
        accept = m["liblz4"] == "accept" or name in ("bad_short_of_csize", "bad_past_csize")   # (the size field is the host's)
        if accept != (list(st) == [0] * len(st)) or not all(int(x) in (0, S.ST_BAD_BLOCK) for x in st):
            bad.append((name, "liblz4 says " + m["liblz4"], list(st)))
        elif list(st) != list(st_e) or list(rl) != list(rl_e):
            bad.append((name, list(st), list(st_e)))
        elif m["liblz4"] == "accept" and (out != e["content"] or list(bl) != list(bl_e)):
            bad.append((name, "content"))
        elif m["liblz4"] == "accept" and (e["frame"][4] & 8) and \
                H.oracle_decompress(S.record(e["frame"]), len(out) + 64) != out:
            bad.append((name, "oracle"))      # (frames with a content size: the oracle's record decode takes them)
    assert not bad, bad


@pytest.mark.skipif(not T.HAVE_LIBLZ4, reason="liblz4 not on this box")
def test_block_kernel_linked_history(eng):
    data = cases.text(600000, 9)
    info = B.walk(H.liblz4_frame(data, block_id=4, linked=1))
    k = len(info["blocks"]) // 2
    s1, b1, r1, o1 = B.tables(dict(info, blocks=info["blocks"][:k]))
    out1, _, rl1, st1 = eng.lz4_decompress_blocks(s1, b1, r1, o1)
    n1 = int(rl1[0])
    assert list(st1) == [0] and out1[:n1] == data[:n1]
    s2, b2, r2, o2 = B.tables(dict(info, blocks=info["blocks"][k:]), history=65536)
    out2, _, rl2, st2 = eng.lz4_decompress_blocks(s2, b2, r2, o2, history=data[n1 - 65536:n1])
    assert list(st2) == [0] and out2[65536:65536 + int(rl2[0])] == data[n1:]
    r2["low"] = r2["out_off"]
    _, _, _, st3 = eng.lz4_decompress_blocks(s2, b2, r2, o2, history=data[n1 - 65536:n1])
    assert list(st3) == [S.ST_BAD_BLOCK]


@pytest.mark.parametrize("n", [0, 15, 16, 33, 70001, 5 << 20])
def test_xxh32_carried_state(eng, n):
    data = cases.rnd(n, n + 3)
    want = xxhash.xxh32(data, seed=0).intdigest()
    for pieces in ([n], [n // 2, n - n // 2], [min(n, 3), max(n - 3, 0)], [min(n, 16), 0, max(n - 16, 0)]):
        assert eng.xxh32_carry(data, pieces) == want, pieces


# ---- 8. a frame above 2 GiB -------------------------------------------------------------------------------------------
class HashIO(H.MemIO):
    """MemIO that keeps a SHA-256 of what is written instead of the bytes"""

    def __init__(self, data):
        super().__init__(data)
        self.sha = hashlib.sha256()
        self.nout = 0
        self._wr = H.RD_FN(self._hash)
        self.rdwr = H.RefRdWr(self._rd, None, self._wr, None)

    def _hash(self, _arg, bufp):
        b = bufp.contents
        self.sha.update(C.string_at(b.buf, b.size))
        self.nout += b.size
        return 0


@pytest.mark.skipif(not T.HAVE_LIBLZ4, reason="liblz4 not on this box")
@pytest.mark.parametrize("linked", [0, 1])
def test_frame_above_2_gib(lib, linked):
    """about 2.2 GiB of text in one frame, with the lz4 tool's defaults (4 MiB independent blocks, content checksum, no
    content size) and with linked blocks; then the same frame with one bit of its content checksum flipped"""
    piece = cases.text(275 << 20, seed=50 + linked)
    data = piece * 8 + b"the end"
    assert len(data) > (2 << 30) + (100 << 20)
    want = hashlib.sha256(data).hexdigest()
    fr = H.liblz4_frame(data, block_id=7, linked=linked, content_size=0, checksum=1)
    n = len(data)
    del data, piece
    for flip in (0, 1):
        st = fr if not flip else fr[:-1] + bytes([fr[-1] ^ 0x10])
        io = HashIO(st)
        ctx = lib.LZ4MT_createDCtx(4, 1 << 20)
        rv = lib.LZ4MT_decompressDCtx(ctx, C.byref(io.rdwr))
        stats = (lib.LZ4MT_GetFramesDCtx(ctx), lib.LZ4MT_GetInsizeDCtx(ctx), lib.LZ4MT_GetOutsizeDCtx(ctx))
        lib.LZ4MT_freeDCtx(ctx)
        if flip:
            assert rv == B.ERR(B.E_LIB)
        else:
            assert rv == 0, lib.LZ4MT_getErrorString(rv)
            assert stats == (0, len(st), n)
            assert io.nout == n and io.sha.hexdigest() == want


# ---- 9. the command line tools ----------------------------------------------------------------------------------------
def test_cli_decodes_plain_lz4_files(tmp_path):
    blocks = [T.SEQ] * 600
    fr = S.frame(blocks, indep=True, csize=False, ccheck=True, bd=7)
    want = S.content(blocks, True)
    f = tmp_path / "small.lz4"
    f.write_bytes(fr)
    r = subprocess.run([os.path.join(BIN, "lz4-mt"), "-d", str(f)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-300:]
    assert (tmp_path / "small").read_bytes() == want
    r = subprocess.run([os.path.join(BIN, "lz4cat-mt")], input=S.frame(blocks, csize=False, bd=7), capture_output=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout == S.content(blocks)
    if T.HAVE_LIBLZ4:
        data = cases.text(60 << 20, seed=12)
        big = tmp_path / "big.lz4"
        big.write_bytes(H.liblz4_frame(data, block_id=7, linked=0))
        env = dict(os.environ, GPUMT_BATCH_MB="16")
        r = subprocess.run([os.path.join(BIN, "lz4-mt"), "-d", "-c", str(big)], capture_output=True, env=env, timeout=300)
        assert r.returncode == 0 and r.stdout == data
