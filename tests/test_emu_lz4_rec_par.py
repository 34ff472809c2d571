"""Multi-block lz4-mt records through the block stages (gpumt_lz4_decompress_batch_par: the kernels of lz4_dec_rec.h in
front of gpumt_lz4_decompress_blocks_par / _seg), on the CPU under the fiber emulator, against gpumt_lz4_decompress_batch on
the same batch (status, d_out_len, bytes of the records that decoded) and against an independent truth: the sequence lists'
plain decode, the committed manifests' SHA-256 and liblz4's recorded verdicts.  tests/test_gpu_lz4_rec_par.py runs the same
cases on the device: the test functions take what differs (`serial`, `par`, `compress`) as fixtures.  lz4_rec_min_blocks is
2 unless a test says otherwise.  No case may hide a fallback: every record a case marks as eligible and clean must come back
with rec_par == its block count."""
import json
import os
import subprocess
import sys

import pytest

import emu_driver as E
import helpers as H
import lz4_rec as K
import lz4_synth as S
from golden import cases


@pytest.fixture(scope="module")
def serial():
    return K.emu_serial


@pytest.fixture(scope="module")
def par():
    return K.emu_par


@pytest.fixture(scope="module")
def compress():
    def oracle(data, chunk, level=1):
        return H.oracle_compress(data, chunk) if level == 1 else H.oracle_compress_level(data, chunk, level)
    return oracle


def records_of(stream):
    ro, rl = E.walk_records(stream)
    return [stream[int(o):int(o) + int(n)] for o, n in zip(ro, rl)]


def content_size(rec):
    return int.from_bytes(rec[18:26], "little") if rec[16] & 0x08 else 0


def clean(got, stats, par, blocks, slices=1, route="par"):
    assert got.stats["par"] == par and got.stats["blocks"] == blocks and got.stats["slices"] == slices
    assert got.stats["fallback"] == 0 and got.stats["route"] == route and got.stats["records"] == len(got.batch)


# ---- the manifest of the hand-built frames ---------------------------------------------------------------------------------
def test_hand_built_frames_are_the_recorded_ones():
    man = K.rec_manifest()["cases"]
    frames = K.manifest_frames()
    assert sorted(man) == sorted(frames)
    for name, fr in frames.items():
        assert S.sha256(fr) == man[name]["frame_sha256"], name
    for name in K.HAND_ELIGIBLE + K.HAND_OTHER:
        assert man[name]["liblz4"] == "accept" and man[name]["content_sha256"] == S.sha256(K.hand(name)[1]), name
    for name in K.HAND_ERRORS:
        assert man[name]["liblz4"] == "reject", name
    assert all(man["edge_" + k]["liblz4"] == "reject" for k in K.edge_frames())


# ---- 1. committed records ---------------------------------------------------------------------------------------------------
def test_committed_records(serial, par):
    with open(os.path.join(H.GOLDEN_DIR, "manifest.json")) as f:
        streams = json.load(f)["cases"]
    with open(os.path.join(H.GOLDEN_DIR, "lz4f_flags", "manifest.json")) as f:
        flags = json.load(f)["cases"]
    recs, owner = [], []
    for fn in sorted(os.listdir(os.path.join(H.GOLDEN_DIR, "streams"))):
        if fn.endswith(".lz4mt"):
            with open(os.path.join(H.GOLDEN_DIR, "streams", fn), "rb") as f:
                for r in records_of(f.read()):
                    recs.append(r)
                    owner.append(("stream", fn[:-6]))
    for fn in sorted(os.listdir(os.path.join(H.GOLDEN_DIR, "lz4f_flags"))):
        if fn.endswith(".rec"):
            with open(os.path.join(H.GOLDEN_DIR, "lz4f_flags", fn), "rb") as f:
                recs.append(f.read())
                owner.append(("flags", fn[:-4]))
    b = K.Batch([(r, content_size(r)) for r in recs])
    ref, got = K.check(b, serial, par)
    assert list(got.status) == [0] * len(b)
    # contents: the manifests' SHA-256
    whole = {}
    for i, (kind, name) in enumerate(owner):
        if kind == "flags":
            assert S.sha256(got.bytes_of(i)) == flags[name]["content_sha256"], name
        else:
            whole[name] = whole.get(name, b"") + got.bytes_of(i)
    for name, data in whole.items():
        assert S.sha256(data) == streams[name]["in_sha256"], name
    # routes: the linked records of two blocks and more took the block stages, every other record did not
    npar = nblk = 0
    for i, (kind, name) in enumerate(owner):
        fr = recs[i][12:]
        n, linked = K.nblocks(fr), not fr[4] & 0x20
        if linked and n >= 2:
            assert int(got.rec_par[i]) == n, (name, n)
            npar, nblk = npar + 1, nblk + n
        else:
            assert int(got.rec_par[i]) == 0, name
    by_name = {name: int(got.rec_par[i]) for i, (kind, name) in enumerate(owner) if kind == "flags"}
    assert by_name["bcheck_text_300k"] == 5 and by_name["dictid_text_150k"] == 3 and by_name["bcheck_indep_text_200k"] == 0
    assert any(K.nblocks(r[12:]) == 1 for r in recs)
    clean(got, got.stats, npar, nblk)


# ---- 2. hand-built mixed batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1], ids=["split", "frame_serial"])
def test_hand_built_records_in_one_mixed_batch(serial, par, variant):
    """variant 1: the record decoders are the wave-per-record kernel alone, which has to pass the kept records by too"""
    man = K.rec_manifest()["cases"]
    b, names = K.mixed_batch()
    ref = serial(b, variant)
    got = par(b, variant)
    assert list(got.status) == list(ref.status) and list(got.out_len) == list(ref.out_len) and got.gaps_intact()
    assert len({int(o) % 4 for o in b.out_off}) == 4, "the output ranges do not start at every alignment"
    npar = nblk = 0
    for i, name in enumerate(names):
        if name in K.HAND_ELIGIBLE:
            fr, want, n = K.hand(name)
            assert int(got.status[i]) == 0 and got.bytes_of(i) == want == ref.bytes_of(i), name
            assert int(got.rec_par[i]) == n, name
            npar, nblk = npar + 1, nblk + n
        elif name in K.HAND_ERRORS:
            assert int(got.status[i]) == K.ST_BAD_BLOCK and man[name]["liblz4"] == "reject" and int(got.rec_par[i]) == 0, name
            npar, nblk = npar + 1, nblk + K.hand(name)[2]           # eligible: the run decoders find the error
        elif name in K.HAND_OTHER:
            assert int(got.status[i]) == 0 and got.bytes_of(i) == K.hand(name)[1] and int(got.rec_par[i]) == 0, name
        else:
            want_st = K.ST_BAD_RECORD if name == "bad_magic" else K.ST_BAD_FRAME
            assert int(got.status[i]) == want_st and int(got.rec_par[i]) == 0, name
    clean(got, got.stats, npar, nblk)


# ---- 3. frame-level edges ---------------------------------------------------------------------------------------------------
def test_frame_level_edges(serial, par):
    edges = K.edge_records()
    fr, want, n = K.hand(K.EDGE)
    names = list(edges) + ["good"]
    b = K.Batch(list(edges.values()) + [(S.record(fr), len(want))])
    ref, got = K.check(b, serial, par)
    st = {name: int(got.status[i]) for i, name in enumerate(names)}
    rp = {name: int(got.rec_par[i]) for i, name in enumerate(names)}
    assert st["good"] == 0 and rp["good"] == 3 and got.bytes_of(len(names) - 1) == want
    assert st["content_size_plus_1"] == K.ST_SIZE_MISMATCH and st["out_len_differs"] == K.ST_SIZE_MISMATCH
    assert st["content_size_minus_1"] != 0
    assert st["content_checksum_flipped"] == K.ST_BAD_CHECKSUM and st["block_checksum_flipped"] == K.ST_BAD_CHECKSUM
    assert st["trailing_byte"] == K.ST_TRAILING and st["record_csize_plus_1"] == K.ST_BAD_RECORD
    assert st["no_end_mark"] != 0 and st["last_block_truncated"] != 0
    # only a record whose blocks and frame are whole was kept: the one whose content checksum alone is wrong
    for name in edges:
        assert rp[name] == (3 if name == "content_checksum_flipped" else 0), name


# ---- 4. slices --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_blocks,slices", [(4, 6), (6, 3), (65536, 1)])
def test_slices(serial, par, slice_blocks, slices):
    """every slice starts behind the first 256 bytes of d_stream and d_out, the later ones at other multiples of 256 than
    the first: a slice base that is not subtracted shows"""
    b, wants = K.slice_batch(lead=600)
    assert int(b.rec_off[0]) >= 512 and int(b.out_off[0]) >= 512
    assert int(b.rec_off[5]) // 256 > int(b.rec_off[0]) // 256 and int(b.out_off[5]) // 256 > int(b.out_off[0]) // 256
    ref, got = K.check(b, serial, par, slice_blocks=slice_blocks)
    assert list(got.status) == [0] * 6 and [int(x) for x in got.rec_par] == [3] * 6
    assert [got.bytes_of(i) for i in range(6)] == wants
    clean(got, got.stats, 6, 18, slices=slices)


def test_a_record_of_more_blocks_than_a_slice_is_a_slice_of_its_own(serial, par):
    fr, want, n = K.hand("five_blocks")
    three = K.n_block_record(3)
    b = K.Batch([(three[0], three[1]), (S.record(fr), len(want)), (three[0], three[1])])
    ref, got = K.check(b, serial, par, slice_blocks=2)
    assert list(got.status) == [0] * 3 and [int(x) for x in got.rec_par] == [3, 5, 3] and got.bytes_of(1) == want
    clean(got, got.stats, 3, 11, slices=3)


# ---- 5. seg route -----------------------------------------------------------------------------------------------------------
def test_seg_route(serial, par):
    one, want1 = K.seg_one_block()
    big, want2 = K.seg_big_blocks()
    assert big[5] == 0x70 and K.nblocks(big) == 2 and K.nblocks(one) == 1
    b = K.Batch([(S.record(one), len(want1)), (S.record(big), len(want2))])
    ref, got = K.check(b, serial, par, seg=1, seg_bytes=256)
    assert list(got.status) == [0, 0] and got.bytes_of(0) == want1 and got.bytes_of(1) == want2
    assert [int(x) for x in got.rec_par] == [1, 2]
    clean(got, got.stats, 2, 3, route="seg")
    # the par route: the one-block record is the record decoders', with the same bytes
    ref, off = K.check(b, serial, par, seg=0, seg_bytes=256)
    assert list(off.status) == [0, 0] and [int(x) for x in off.rec_par] == [0, 2] and (off.area == got.area).all()
    clean(off, off.stats, 1, 2, route="par")


# ---- 6. live streams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,chunk,level,seed", [(300 * 1024, 1 << 20, 1, 5), (900 * 1024, 400000, 1, 67),
                                                   (300 * 1024, 1 << 20, 9, 9)], ids=["300k", "900k_3rec", "level9"])
def test_live_streams(serial, par, compress, size, chunk, level, seed):
    data = cases.text(size, seed)
    stream = compress(data, chunk, level)
    recs = records_of(stream)
    counts = [K.nblocks(r[12:]) for r in recs]
    assert counts == [(min(chunk, size - i) + 65535) // 65536 for i in range(0, size, chunk)]
    b = K.Batch([(r, content_size(r)) for r in recs])
    ref, got = K.check(b, serial, par)
    assert list(got.status) == [0] * len(b) and b"".join(got.bytes_of(i) for i in range(len(b))) == data
    assert [int(x) for x in got.rec_par] == counts
    clean(got, got.stats, len(b), sum(counts))


# ---- 7. default threshold, switch off, scratch cap --------------------------------------------------------------------------
def test_default_threshold(serial, par):
    d = K.DEFAULT_MIN_BLOCKS
    below, at = K.n_block_record(d - 1), K.n_block_record(d)
    b = K.Batch([(below[0], below[1]), (at[0], at[1])])
    ref, got = K.check(b, serial, par, min_blocks=None)
    assert [int(x) for x in got.rec_par] == [0, d] and list(got.status) == [0, 0]
    assert got.bytes_of(0) == below[2] and got.bytes_of(1) == at[2]


def test_switch_off(serial, par):
    b, wants = K.slice_batch()
    ref, got = K.check(b, serial, par, rec_par=0)
    assert not any(got.rec_par) and list(got.status) == [0] * 6
    clean(got, got.stats, 0, 0, slices=0)


def test_scratch_cap_falls_back(serial, par):
    """a cap of 1 MiB: a batch whose block table alone is larger goes to the record decoders, a later small one does not"""
    big = K.many_blocks_batch()
    ref, got = K.check(big, serial, par, slice_blocks=65536, cap_mb=1)
    assert got.stats["fallback"] == 1 and got.stats["par"] == 0 and not any(got.rec_par)
    assert list(got.status) == [0] * len(big)
    b, wants = K.slice_batch()
    ref, got = K.check(b, serial, par, cap_mb=1)
    assert [int(x) for x in got.rec_par] == [3] * 6 and list(got.status) == [0] * 6
    clean(got, got.stats, 6, 18)


# ---- 8. interleaved calls ---------------------------------------------------------------------------------------------------
def test_interleaved_calls_on_one_stream(serial, par):
    """par, the plain call, par with a larger batch, the plain call again: the two carve up the same scratch"""
    small, wants = K.slice_batch()
    fr, want, n = K.hand("full_64k_then_65535")
    big_recs = [(S.record(fr), len(want))] * 3 + list(small.records)
    big = K.Batch(big_recs)
    a = par(small)
    s1 = serial(big)
    c = par(big)
    s2 = serial(small)
    assert list(a.status) == [0] * 6 and [a.bytes_of(i) for i in range(6)] == wants and [int(x) for x in a.rec_par] == [3] * 6
    assert list(s2.status) == [0] * 6 and [s2.bytes_of(i) for i in range(6)] == wants
    for r in (s1, c):
        assert list(r.status) == [0] * 9 and [r.bytes_of(i) for i in range(9)] == [want] * 3 + wants
        assert r.gaps_intact()
    assert [int(x) for x in c.rec_par] == [2] * 3 + [3] * 6
    clean(c, c.stats, 9, 24)


# ---- the emulator's other lane orders --------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_new_kernels_under_the_strict_and_the_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "mixed_batch or edges or slices or slice_of_its_own or default_threshold"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-1500:]
