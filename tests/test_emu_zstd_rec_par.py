"""Multi-block zstd-mt records through the block stages (gpumt_zstd_decompress_batch_par: the kernels of zstd_dec_rec.h in
front of gpumt_zstd_decompress_blocks_par), on the CPU under the fiber emulator, against gpumt_zstd_decompress_batch on the
same batch: status, d_out_len and bytes.  tests/test_gpu_zstd_rec_par.py runs the same cases on the device: the test
functions take what differs (`serial`, `par`, `kind`) as fixtures.  zstd_rec_min_blocks is 1 unless a test says otherwise."""
import json
import os
import subprocess
import sys

import pytest

import helpers as H
import zstd_blocks as Z
import zstd_par as R
import zstd_rec as K
import zstd_synth as S

with open(os.path.join(H.GOLDEN_DIR, "zstd_synth", "manifest.json")) as _f:
    MAN = json.load(_f)


@pytest.fixture(scope="module")
def serial():
    return K.emu_serial


@pytest.fixture(scope="module")
def par():
    return K.emu_par


@pytest.fixture(scope="module")
def kind():
    return "emu"


# ---- 1. committed records ---------------------------------------------------------------------------------------------------
SEEN = {"par": 0}
MULTI = ("z_text_200k_", "z_zeros_300k", "z_mixed")


@pytest.mark.parametrize("name", K.COMMITTED)
def test_committed_records(serial, par, name):
    frames = K.committed(name)
    b = K.Batch([(S.record(fr), K.cap_of(fr), 0) for fr in frames])
    ref, got = K.check(b, serial, par)
    assert all(int(s) == 0 for s in ref.status)
    counts = [K.nblocks(fr) for fr in frames]
    if name.startswith(MULTI):
        assert max(counts) >= 2, counts
    for i, n in enumerate(counts):
        if n >= 2:
            assert int(got.rec_par[i]) == n, (name, i)
        else:
            assert int(got.rec_par[i]) in (0, n)
    SEEN["par"] += sum(int(x) for x in got.rec_par)


def test_committed_records_took_the_parallel_route(serial, par):
    """d_rec_par is not all zero over the set (run alone, this test decodes one file itself)"""
    if not SEEN["par"]:
        test_committed_records(serial, par, "z_text_200k_l5")
    assert SEEN["par"] > 0


# ---- 2. committed plain frames as records -----------------------------------------------------------------------------------
def plain_batch(flip=None):
    recs, kinds = [], set()
    for name in sorted(Z.FIXTURES):
        fr, plain = Z.fixture(name)
        info = Z.walk(fr)
        kinds.add((info["csize"] is not None, info["cchk"]))
        if flip is not None and info["cchk"]:
            fr = fr[:-1 - flip % 4] + bytes([fr[-1 - flip % 4] ^ 0x10]) + fr[len(fr) - flip % 4:]
        recs.append((S.record(fr), K.cap_of(fr, plain), 0))
    return K.Batch(recs), kinds


def test_plain_frames_as_records(serial, par):
    b, kinds = plain_batch()
    assert (False, False) in kinds or (False, True) in kinds, "no frame without a content size among the fixtures"
    assert (True, True) in kinds, "no frame with checksum and size among the fixtures"
    ref, got = K.check(b, serial, par)
    for i, name in enumerate(sorted(Z.FIXTURES)):
        fr, plain = Z.fixture(name)
        assert int(got.status[i]) == 0 and got.bytes_of(i) == plain, name     # capacity in, size out
        assert int(got.rec_par[i]) == K.nblocks(fr), name


def test_plain_frames_with_a_flipped_checksum_byte(serial, par):
    b, _ = plain_batch(flip=2)
    ref, got = K.check(b, serial, par)
    n = 0
    for i, name in enumerate(sorted(Z.FIXTURES)):
        if Z.walk(Z.fixture(name)[0])["cchk"]:
            assert int(got.status[i]) == int(ref.status[i]) == K.ST_BAD_CHECKSUM, name
            n += 1
        else:
            assert int(got.status[i]) == 0
    assert n > 0


# ---- 3. hand-built frames in one mixed batch --------------------------------------------------------------------------------
def test_hand_built_frames_in_one_mixed_batch(serial, par):
    b, names = K.mixed_batch()
    assert {"one_block", "empty", "preset"} <= set(names) and set(R.HAND_NAMES) <= set(names)
    ref, got = K.check(b, serial, par)
    for i, name in enumerate(names):
        if name == "preset":
            continue
        if name in R.HAND_NAMES:
            fr, want, info = R.hand(name)
            if want is None:
                assert name == "rep_zero_incoming" and int(got.status[i]) == Z.ST_BAD_BLOCK and int(got.rec_par[i]) == 0
            else:
                assert int(got.status[i]) == 0 and got.bytes_of(i) == want, name
                assert int(got.rec_par[i]) == len(info["blocks"]), name
        else:
            assert int(got.status[i]) == 0 and int(got.rec_par[i]) == 1, name
    assert got.stats["par"] == len(names) - 2 and got.stats["fallback"] == 0


# ---- 4. every stream of the zstd_synth manifest -----------------------------------------------------------------------------
def test_synth_streams_as_records(serial, par):
    cases = S.families(MAN["seed"])
    names = sorted(cases)
    assert names == sorted(MAN["cases"])
    b = K.Batch([(S.record(cases[n]["frame"]), K.cap_of(cases[n]["frame"], cases[n]["content"]), 0) for n in names])
    ref, got = K.check(b, serial, par)
    bad = []
    for i, n in enumerate(names):
        m = MAN["cases"][n]
        if m["libzstd"] == "accept" and n not in S.DIVERGENT:
            if int(got.status[i]) != 0 or S.sha256(got.bytes_of(i)) != m["content_sha256"]:
                bad.append((n, int(got.status[i])))
    assert not bad, bad
    assert sum(int(x) for x in got.rec_par) > 0


# ---- 5. frame-level edges ---------------------------------------------------------------------------------------------------
def test_frame_level_edges(serial, par):
    edges = K.edge_records()
    fr, want, _ = R.hand(K.EDGE_FRAME)
    good = K.hand_frame(K.EDGE_FRAME, fcs=0)
    names = list(edges) + ["good", "good_no_size"]
    b = K.Batch([(r, c, 0) for r, c in edges.values()] + [(S.record(fr), len(want), 0), (S.record(good), len(want), 0)])
    ref, got = K.check(b, serial, par)
    for i, n in enumerate(names[:-2]):
        assert int(ref.status[i]) != 0 and int(got.rec_par[i]) == 0, n
    for i in (len(names) - 2, len(names) - 1):
        assert int(got.status[i]) == 0 and int(got.rec_par[i]) == 3 and got.bytes_of(i) == want, names[i]


# ---- 6. damage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_damaged_record(serial, par, part):
    """one bit flipped at 256 positions (fixed seed) of the two-block tiled record, 64 records per batch"""
    b = K.damaged_batch(part)
    ref, got = K.check(b, serial, par)
    assert {int(s) for s in ref.status} - {0}, "no flip of this part was noticed at all"


def test_the_undamaged_record_takes_the_parallel_route(serial, par):
    fr, _, _, cap = K.damage_record()
    ref, got = K.check(K.Batch([(S.record(fr), cap, 0)]), serial, par)
    assert int(got.status[0]) == 0 and int(got.rec_par[0]) == R.DAMAGE_BLOCKS


# ---- 7. slices --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_blocks", [2, 5])
def test_slices(serial, par, slice_blocks):
    b, names = K.slice_batch()
    whole = par(b)
    ref, got = K.check(b, serial, par, slice_blocks=slice_blocks)
    assert got.stats["slices"] > 1 and whole.stats["slices"] == 1
    assert list(got.status) == list(whole.status) == [0] * 7 and (got.area == whole.area).all()
    assert [int(x) for x in got.rec_par] == [int(x) for x in whole.rec_par] == [len(R.hand(x)[2]["blocks"]) for x in names]


# ---- 8. default threshold ---------------------------------------------------------------------------------------------------
def test_default_threshold(serial, par):
    three, four = R.hand(K.EDGE_FRAME), R.hand("straddle")
    assert len(three[2]["blocks"]) == 3 and len(four[2]["blocks"]) == 4
    b = K.Batch([(S.record(three[0]), len(three[1]), 0), (S.record(four[0]), len(four[1]), 0)])
    ref, got = K.check(b, serial, par, min_blocks=None)
    assert [int(x) for x in got.rec_par] == [0, 4] and list(got.status) == [0, 0]


# ---- 9. switches ------------------------------------------------------------------------------------------------------------
def test_switch_off(serial, par):
    b, names = K.slice_batch()
    ref, got = K.check(b, serial, par, rec_par=0)
    assert not any(got.rec_par) and list(got.status) == [0] * 7


def test_scratch_cap_falls_back(serial, par):
    """a cap of 1 MiB: a batch whose block table alone is larger goes to the record decoders, a small one does not"""
    big = K.many_blocks_batch()
    ref, got = K.check(big, serial, par, slice_blocks=65536, cap_mb=1)
    assert got.stats["fallback"] == 1 and not any(got.rec_par) and list(got.status) == [0] * len(big)
    b, names = K.slice_batch()
    ref, got = K.check(b, serial, par, cap_mb=1)
    assert got.stats["fallback"] == 0 and all(got.rec_par) and list(got.status) == [0] * 7


# ---- the emulator's other lane orders --------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_new_kernels_under_the_strict_and_the_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "mixed_batch or edges or slices or default_threshold"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-1500:]
