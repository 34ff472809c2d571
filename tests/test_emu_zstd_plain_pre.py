"""The block-parallel entropy pre-pass in front of the block runs (gpumt_zstd_decompress_blocks_pre: classify, resolve,
entropy and execute kernels of zstd_dec.hip), on the CPU under the fiber emulator, against the serial entry point
gpumt_zstd_decompress_blocks.  tests/test_gpu_zstd_plain_pre.py runs the same cases on the device: the test functions take
what differs (`pre`, `pre_off`, `serial`, `kind`) as fixtures."""
import os
import subprocess
import sys

import pytest

import helpers as H
import zstd_blocks as Z
import zstd_pre as P


@pytest.fixture(scope="module")
def pre():
    return P.emu_decode_blocks_pre


@pytest.fixture(scope="module")
def pre_off():
    return lambda *a, **k: P.emu_decode_blocks_pre(*a, pre_on=0, **k)


@pytest.fixture(scope="module")
def serial():
    return Z.emu_decode_blocks


@pytest.fixture(scope="module")
def kind():
    return "emu"


def test_the_fixtures_hold_every_kind_of_borrowed_table():
    """the mark test below is a condition on treeless literals and on Repeat_Mode of each of LL, OF and ML only if the
    committed streams contain them"""
    assert {"treeless", "repeat_ll", "repeat_of", "repeat_ml"} <= P.fixture_kinds()
    assert {b["type"] for b in P.frame("hand")[2]["blocks"]} == {0, 1, 2}


# ---- 1. + 2. + 3. equality with the serial entry point, the marks, definers before the call ----------------------------
@pytest.mark.parametrize("name,cut", P.cut_params())
def test_equal_to_serial_and_marked(pre, serial, kind, name, cut):
    """one run (cut 0) or two calls with the boundary in front of block `cut`, history and carry between them: bytes,
    run_len, status and the carry left behind are the serial entry point's, the content is the oracle's, and exactly the
    blocks whose tables are their own or defined inside the same call are marked"""
    fr, want, info = P.frame(name)
    ref = P.serial_parts(serial, (kind, name, cut), info, cut)
    got = P.decode_parts(pre, info, cut)
    assert [r[2] for r in ref] == [0] * len(ref)
    assert [g[:4] for g in got] == [r[:4] for r in ref]
    assert b"".join(g[0] for g in got) == want
    if cut == 0:
        assert H.oracle_zstdmt_decompress(H.mt_record(fr), len(want) + 64) == want
    n = len(info["blocks"])
    bounds = [(0, n)] if cut == 0 else [(0, cut), (cut, n)]
    assert [g[4] for g in got] == [P.expected_marks(info, lo, hi) for lo, hi in bounds]


def test_definer_before_the_call_stays_serial(pre, serial, kind):
    """a second call that starts with a treeless block, and one that starts with a Repeat_Mode table of each kind: the
    bit of what the block borrows is clear (the table is in the carry), the blocks behind it are marked again once a
    block of the call describes the table, and the output is the serial one"""
    seen = set()
    for name in ("l1_plain", "l19_tiled"):
        fr, want, info = P.frame(name)
        for cut, kinds in Z.cut_kinds(info).items():
            new = kinds & {"treeless", "repeat_ll", "repeat_of", "repeat_ml"}
            if not new or new <= seen:
                continue
            seen |= new
            got = P.decode_parts(pre, info, cut)
            assert [g[:4] for g in got] == [r[:4] for r in P.serial_parts(serial, (kind, name, cut), info, cut)]
            first = got[1][4][0]
            assert (first & P.LIT == 0) == ("treeless" in kinds), (name, cut)
            assert (first & P.SEQ == 0) == bool(kinds & {"repeat_ll", "repeat_of", "repeat_ml"}), (name, cut)
    assert seen == {"treeless", "repeat_ll", "repeat_of", "repeat_ml"}


def test_several_runs_side_by_side(pre, serial):
    """two frames in one call, the second one's blocks behind the first one's in the table: a definer is looked for in
    the block's own run only"""
    import numpy as np
    from zstdmt_amd.device import ZSTD_BLOCK, ZSTD_RUN
    (_, w1, i1), (_, w2, i2) = P.frame("l1_plain"), P.frame("l19_tiled")
    i2 = dict(i2, blocks=i2["blocks"][2:5])          # starts with a Repeat_Mode block: nothing to take the table from
    s1, b1, r1, o1 = Z.tables(i1, 0, len(i1["blocks"]))
    s2, b2, r2, o2 = Z.tables(i2, 0, 3)
    b2 = b2.copy()
    b2["src_off"] += len(s1)
    r2 = r2.copy()
    r2["first"], r2["out_off"], r2["flags"] = len(b1), o1, Z.ZRUN_FIRST | Z.ZRUN_LAST
    blocks, runs = np.concatenate([b1, b2]).astype(ZSTD_BLOCK), np.concatenate([r1, r2]).astype(ZSTD_RUN)
    ref = serial(s1 + s2, blocks, runs, o1 + o2)
    got = pre(s1 + s2, blocks, runs, o1 + o2)
    assert list(ref[2]) == [0, Z.ST_BAD_BLOCK] and ref[0][:len(w1)] == w1
    assert (got[0], list(got[1]), list(got[2])) == (ref[0], list(ref[1]), list(ref[2]))
    assert list(got[4]) == P.expected_marks(i1, 0, len(i1["blocks"])) + P.expected_marks(i2, 0, 3)
    assert got[4][len(b1)] & P.SEQ == 0


# ---- 4. verdict parity on damaged input ----------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["headers", "sample0", "sample1", "sample2"])
@pytest.mark.parametrize("name", ["l1_plain", "l19_plain"])
def test_damaged_input_gets_the_serial_verdict(pre, serial, kind, name, group):
    """the first two blocks of a level-1 and of a level-19 stream as one run that goes on, one bit flipped: status,
    run_len, the bytes decoded and the carry are the serial entry point's for every flip (and nothing is written behind
    the output: the decode functions check their 64 guard bytes).  The sample is 24 positions under the emulator and 768
    on the device (zstd_pre.SAMPLES), a third of them per group"""
    info = P.frame(name)[2]
    s, b, r, o = Z.tables(info, 0, 2)
    verdicts = set()
    for pos, bit in P.flips(info, 2, group, P.SAMPLES[kind]):
        bad = bytearray(s)
        bad[pos] ^= bit
        ref = serial(bytes(bad), b, r, o)
        got = pre(bytes(bad), b, r, o)
        n = int(ref[1][0])
        assert (int(got[2][0]), int(got[1][0])) == (int(ref[2][0]), n), (pos, bit)
        assert got[0][:n] == ref[0][:n], (pos, bit)
        assert P.carry_state(got[3], 0) == P.carry_state(ref[3], 0), (pos, bit)
        verdicts.add(int(ref[2][0]))
    assert verdicts - {0}, "no flip of this group was noticed at all"


# ---- 5. the knob ---------------------------------------------------------------------------------------------------------
def test_knob_off_marks_nothing(pre_off, serial, kind):
    for name in ("l3_plain", "hand"):
        fr, want, info = P.frame(name)
        got = P.decode_parts(pre_off, info, 2)
        assert [g[:4] for g in got] == [r[:4] for r in P.serial_parts(serial, (kind, name, 2), info, 2)]
        assert all(m == 0 for g in got for m in g[4])


# ---- the emulator's other lane orders --------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_new_kernels_under_the_strict_and_the_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "(equal_to_serial and (l19_tiled or l1_plain or hand)) or definer_before or side_by_side or (damaged and headers)"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-1500:]
