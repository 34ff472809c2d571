"""The entropy pre-pass under ZSTDCB_decompressDCtx (mt_zstd_plain.inc over gpumt_zstd_decompress_blocks_pre), on the CPU
over the emulated device: single frames of about 1 MiB at levels 1, 3 and 19 over 64 KiB batches, with the pre-pass on and
off.  tests/test_gpu_zstd_plain_pre_api.py runs the same cases on the device."""
import hashlib

import pytest

import zstd_blocks as Z
import zstd_pre as P
import zstd_pre_api as A


@pytest.fixture(scope="module")
def on():
    return A.run_api("emu", True)


@pytest.fixture(scope="module")
def off():
    return A.run_api("emu", False)


@pytest.fixture(scope="module")
def wide():
    """batches of 512 KiB, several blocks each, pre-pass on and off; and a value of the variable that is neither"""
    only = ["level3", "level19"]
    return (A.run_api("emu", True, 512, only), A.run_api("emu", False, 512, only), A.run_api("emu", "2", 512, ["level3"]))


@pytest.mark.parametrize("name", ["level1", "level3", "level19"])
def test_same_content_trace_and_counters_on_and_off(on, off, name):
    st, want = A.api_cases()[name]
    a, b = on[name], off[name]
    assert a["rv"] == 0 and a["nout"] == len(want) and a["sha"] == hashlib.sha256(want).hexdigest()
    assert a["stats"] == [0, len(st), len(want)]
    assert a["batches"] >= 3
    for key in ("rv", "sha", "nout", "stats", "reads", "writes", "batches", "blocks"):
        assert a[key] == b[key], key
    # the frame carries a content checksum: it verified either way; and the pre-pass did run, or did not
    assert Z.walk(st)["cchk"]
    assert a["pre_seq"] > a["blocks"] // 2 and a["pre_lit"] > a["blocks"] // 2
    assert b["pre_seq"] == 0 and b["pre_lit"] == 0


def test_wrong_checksum_is_refused_with_the_same_code(on, off):
    assert on["err_wrong_checksum"]["rv"] == off["err_wrong_checksum"]["rv"] == Z.ERR(Z.E_LIB)
    assert on["err_wrong_checksum"]["pre_seq"] > 0


@pytest.mark.parametrize("name", ["level3", "level19"])
def test_batches_of_several_blocks(on, wide, name):
    """with 512 KiB of input per batch a block that borrows a table finds the block that describes it inside the same
    call: same content, trace and counters on and off, and no block fewer decoded ahead than with one block per batch"""
    st, want = A.api_cases()[name]
    a, b = wide[0][name], wide[1][name]
    assert a["rv"] == 0 and a["sha"] == hashlib.sha256(want).hexdigest() and a["batches"] < a["blocks"]
    for key in ("rv", "sha", "nout", "stats", "reads", "writes", "batches", "blocks"):
        assert a[key] == b[key], key
    assert a["pre_seq"] >= on[name]["pre_seq"] and a["pre_lit"] >= on[name]["pre_lit"]
    if a["batches"] == 1:   # the whole frame in one call: the header walk of zstd_pre.py says which blocks are marked
        info = Z.walk(st)
        marks = P.expected_marks(info, 0, len(info["blocks"]))
        assert (a["pre_seq"], a["pre_lit"]) == (sum(m & P.SEQ for m in marks), sum(m & P.LIT for m in marks) // P.LIT)
    assert b["pre_seq"] == 0 and b["pre_lit"] == 0
    assert wide[0]["knob"] == wide[1]["knob"] == []


def test_other_values_of_the_variable_are_ignored(wide):
    """neither 0 nor 1: the host engine's default, which is the serial call, with the same content; the device boundary
    says that it ignored the value"""
    b, c = wide[1]["level3"], wide[2]["level3"]
    assert c["rv"] == 0 and (c["sha"], c["pre_seq"], c["pre_lit"]) == (b["sha"], 0, 0)
    assert all("GPUMT_ZSTD_RUN_PRE=2 ignored" in k for k in wide[2]["knob"]) and len(wide[2]["knob"]) <= 1
