"""The block-parallel execute stage behind the entropy pre-pass (gpumt_zstd_decompress_blocks_par: the kernels of
zstd_dec_par.h), on the CPU under the fiber emulator, against the serial entry point gpumt_zstd_decompress_blocks.
tests/test_gpu_zstd_plain_par.py runs the same cases on the device: the test functions take what differs (`par`,
`par_off`, `pre`, `serial`, `kind`) as fixtures."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import zstd_blocks as Z
import zstd_pre as P
import zstd_par as R
from zstdmt_amd.device import ZSTD_BLOCK, ZSTD_RUN


@pytest.fixture(scope="module")
def par():
    return R.emu_decode_blocks_par


@pytest.fixture(scope="module")
def par_off():
    return lambda *a, **k: R.emu_decode_blocks_par(*a, par_on=0, **k)


@pytest.fixture(scope="module")
def pre():
    return P.emu_decode_blocks_pre


@pytest.fixture(scope="module")
def serial():
    return Z.emu_decode_blocks


@pytest.fixture(scope="module")
def kind():
    return "emu"


def cuts_of(kind, n):
    return list(range(n)) if kind == "emu" else R.thin(range(n))


SEEN = {"prefix_and_suffix": 0, "fully_parallel": 0}


def check_cut(par, pre, serial, kind, key, info, want, cut):
    """two calls (one for cut 0) through par/par, serial/par and par/serial: everything a caller sees is the serial
    call's, the marks are the pre call's, block_par is what the marks say"""
    n = len(info["blocks"])
    bounds = [(0, n)] if cut == 0 else [(0, cut), (cut, n)]
    ref = R.decode_parts([serial, serial], info, cut)
    marks = [g[4] for g in R.decode_parts([pre, pre], info, cut)]
    for decs in ([par, par], [serial, par], [par, serial])[:3 if cut else 1]:
        got = R.decode_parts(decs, info, cut)
        assert [g[:4] for g in got] == [r[:4] for r in ref], (key, cut)
        if want is not None:
            assert b"".join(g[0] for g in got) == want
        for g, m, d, (lo, hi) in zip(got, marks, decs, bounds):
            if d is par:
                exp, s = R.expected_par(info, lo, hi)
                if g[2] != 0:
                    exp = [0] * (hi - lo)      # a failing run is the serial wave's: nothing of the parallel stage is kept
                assert g[4] == m == P.expected_marks(info, lo, hi) and g[5] == exp, (key, cut, lo, hi)
                if any(exp):
                    SEEN["prefix_and_suffix" if s else "fully_parallel"] += 1


# ---- 1. every committed stream at every cut -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.FIXTURE_NAMES)
def test_committed_streams_at_every_cut(par, pre, serial, kind, name):
    fr, want, info = P.frame(name)
    for cut in cuts_of(kind, len(info["blocks"])):
        check_cut(par, pre, serial, kind, name, info, want, cut)


def test_the_decoder_reported_both_kinds_of_run(par, pre, serial, kind):
    """what the calls above reported in d_block_par, not what the headers promise: a run with a serial prefix and a
    parallel suffix, and a fully parallel one.  (Run alone, this test decodes the tiled stream at two cuts itself.)"""
    if not (SEEN["prefix_and_suffix"] and SEEN["fully_parallel"]):
        fr, want, info = P.frame("l19_tiled")
        for cut in (0, 2):
            check_cut(par, pre, serial, kind, "l19_tiled", info, want, cut)
    assert SEEN["prefix_and_suffix"] > 0 and SEEN["fully_parallel"] > 0, SEEN


def test_the_fixtures_show_both_kinds_of_run():
    """over all committed streams and cuts there is a run with a serial prefix and a parallel suffix, and a fully parallel
    one (computed from the headers alone, so the test above cannot pass quietly without either)"""
    seen = set()
    for name in P.FIXTURE_NAMES:
        info = P.frame(name)[2]
        n = len(info["blocks"])
        for cut in range(n):
            for lo, hi in ([(0, n)] if cut == 0 else [(0, cut), (cut, n)]):
                exp, s = R.expected_par(info, lo, hi)
                if any(exp):
                    seen.add("prefix" if s else "full")
    assert seen == {"prefix", "full"}


# ---- 2. hand-built frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.HAND_NAMES)
def test_hand_built_frames_at_every_cut(par, pre, serial, kind, name):
    fr, want, info = R.hand(name)
    n = len(info["blocks"])
    ref = R.decode_parts([serial], info, 0)
    if want is None:
        assert ref[0][2] == Z.ST_BAD_BLOCK
    else:
        assert ref[0][2] == 0 and ref[0][0] == want
    for cut in range(n):
        check_cut(par, pre, serial, kind, name, info, want, cut)


def test_dense_block_moves_the_split(par):
    info = R.hand("dense_middle")[2]
    assert R.expected_par(info, 0, 5) == ([0, 0, 0, 1, 1], 3)
    assert R.decode_parts([par], info, 0)[0][5] == [0, 0, 0, 1, 1]


def test_history_edge(par, serial):
    """a source at the first byte of the history is read; one byte in front of it is BAD_BLOCK, as in the serial call"""
    fr, want, info = R.hand("back_1_2_3")
    head = want[:900]                                      # blocks 3 and 4 reach 800 and 1000 bytes back
    t = Z.tables(info, 0, 3)
    cy = serial(*t)[3]                                     # what the frame's first three blocks leave behind
    trace = []
    R.S.content(R.hand_blocks()["back_1_2_3"], block_max=1024, trace=trace)
    for hi, end in ((4, 972), (5, len(want))):
        need = 900 - min(pos - off for pos, off in trace if 900 <= pos < end)     # the history the run's deepest match needs
        assert 700 < need <= 900
        for hist, status in ((900, 0), (need + 1, 0), (need, 0), (need - 1, Z.ST_BAD_BLOCK)):
            ref = R.one_run(serial, info, 3, hi, head[900 - hist:], carry=cy)
            got = R.one_run(par, info, 3, hi, head[900 - hist:], carry=cy)
            assert ref[2] == status and got[:4] == ref[:4], (hi, hist)
            if hi == 5:
                assert got[4] == ([1, 1] if status == 0 else [0, 0])


def test_output_one_byte_short(par, serial):
    for name in ("back_1_2_3", "raw_rle_between", "no_sequences"):
        fr, want, info = R.hand(name)
        n = len(info["blocks"])
        ref, got = R.one_run(serial, info, 0, n, b"", len(want) - 1), R.one_run(par, info, 0, n, b"", len(want) - 1)
        assert ref[2] != 0 and got[:4] == ref[:4] and not any(got[4]), name
        ref, got = R.one_run(serial, info, 0, n, b"", len(want)), R.one_run(par, info, 0, n, b"", len(want))
        assert ref[2] == 0 and got[:4] == ref[:4] and all(got[4]), name


def test_damaged_block_in_the_middle(par, serial):
    """bits flipped in the third block of a run of good ones: verdict, run_len and the bytes before the failure"""
    fr, want, info = R.hand("back_1_2_3")
    base = sum(len(b["raw"]) for b in info["blocks"][:3])
    seen = set()
    for at, bit in [(0, 2), (0, 4), (1, 1), (3, 8), (4, 1), (6, 16), (9, 1), (12, 128), (20, 4), (25, 1)]:
        ref = R.one_run(serial, info, 0, 5, b"", damage=(base + at, bit))
        got = R.one_run(par, info, 0, 5, b"", damage=(base + at, bit))
        assert got[:4] == ref[:4], (at, bit)
        seen.add(ref[2])
    assert seen - {0}


def test_two_runs_on_two_carry_slots(par, serial):
    """a good run on slot 0 and a failing one on slot 1 in one call"""
    (_, w1, i1), (_, _, i2) = R.hand("rep_ll_zero"), R.hand("rep_zero_incoming")
    s1, b1, r1, o1 = Z.tables(i1, 0, 4)
    s2, b2, r2, o2 = Z.tables(i2, 0, 5)
    b2, r2 = b2.copy(), r2.copy()
    b2["src_off"] += len(s1)
    r2["first"], r2["out_off"], r2["carry"] = len(b1), o1, 1
    r1, r2 = r1.copy(), r2.copy()
    r1["flags"], r2["flags"] = Z.ZRUN_FIRST, Z.ZRUN_FIRST
    blocks, runs = np.concatenate([b1, b2]).astype(ZSTD_BLOCK), np.concatenate([r1, r2]).astype(ZSTD_RUN)
    ref, got = serial(s1 + s2, blocks, runs, o1 + o2), par(s1 + s2, blocks, runs, o1 + o2)
    assert list(ref[2]) == [0, Z.ST_BAD_BLOCK]
    assert (list(got[1]), list(got[2])) == (list(ref[1]), list(ref[2]))
    n1, n2 = int(ref[1][0]), int(ref[1][1])
    assert got[0][:n1] == ref[0][:n1] and got[0][o1:o1 + n2] == ref[0][o1:o1 + n2]
    assert P.carry_state(got[3], 0) == P.carry_state(ref[3], 0)
    assert P.carry_state(got[3], 1)[4] == P.carry_state(ref[3], 1)[4] == 1
    assert list(got[5]) == [1] * 4 + [0] * 5


# ---- 3. damaged committed stream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_damaged_committed_stream(par, serial, kind, part):
    """one bit flipped at 256 positions (fixed seed) of the first two blocks of the tiled stream (a run of two fully marked
    blocks: the parallel path), 64 per case, on the emulator as on the device: status, run_len, and the bytes and the
    carry the serial call left.  Damaged input is refused, never followed"""
    info = P.frame(R.DAMAGE_FRAME)[2]
    nb = R.DAMAGE_BLOCKS
    assert R.expected_par(info, 0, nb)[0] == [1] * nb
    total = sum(len(b["raw"]) for b in info["blocks"][:nb])
    verdicts = set()
    for pos, bit in R.damage_positions(total)[64 * part:64 * part + 64]:
        ref = R.one_run(serial, info, 0, nb, b"", damage=(pos, bit))
        got = R.one_run(par, info, 0, nb, b"", damage=(pos, bit))
        assert got[1:4] == ref[1:4], (pos, bit)
        assert got[0] == ref[0], (pos, bit)
        verdicts.add(ref[2])
    assert verdicts - {0}, "no flip of this part was noticed at all"


# ---- 4. the switch ---------------------------------------------------------------------------------------------------------
def test_switch_off_is_the_pre_call(par_off, pre, kind):
    for name in ("l19_tiled", "back_1_2_3"):
        info = (P.frame(name) if name in P.FIXTURE_NAMES else R.hand(name))[2]
        got, ref = R.decode_parts([par_off, par_off], info, 2), R.decode_parts([pre, pre], info, 2)
        assert [g[:5] for g in got] == [r[:5] for r in ref]
        assert all(x == 0 for g in got for x in g[5])


# ---- the emulator's other lane orders --------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_new_kernels_under_the_strict_and_the_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "hand_built or history_edge or one_byte_short or damaged_block or two_runs or (committed and l19_tiled)"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-1500:]
