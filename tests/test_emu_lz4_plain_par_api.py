"""Linked-block plain .lz4 frames through LZ4MT_decompressDCtx (mt_lz4_plain.inc over gpumt_lz4_decompress_blocks_par), on
the CPU over the emulated device: frames of many batches with GPUMT_LZ4_RUN_PAR on and off -- same bytes, callback sizes,
counters and final error.  tests/test_gpu_lz4_plain_par_api.py runs the same cases on the device."""
import pytest

import lz4_blocks as B
import lz4_par_api as A

NAMES = sorted(A.api_cases())


@pytest.fixture(scope="module")
def on():
    return A.run_api("emu", True)


@pytest.fixture(scope="module")
def off():
    return A.run_api("emu", False)


@pytest.mark.parametrize("name", NAMES)
def test_same_bytes_callbacks_counters_and_error_on_and_off(on, off, name):
    A.check_on_off(on, off, name, B.ERR(B.E_LIB))
    assert on["knob"] == off["knob"] == []


def test_other_values_of_the_variable(on, off):
    """neither 0 nor 1: the host engine takes its default, the content is the same, and the device boundary says that it
    ignored the value; unset is that default too"""
    odd = A.run_api("emu", "yes", only=["synth_linked"])
    unset = A.run_api("emu", None, only=["synth_linked"])
    for res in (odd, unset):
        for key in A.KEYS:
            assert res["synth_linked"][key] == on["synth_linked"][key], key
    assert odd["synth_linked"]["par"] == unset["synth_linked"]["par"]
    # (the emulated boundary reads the variable where the block-parallel call is first made)
    assert all("GPUMT_LZ4_RUN_PAR=yes ignored" in k for k in odd["knob"]) and len(odd["knob"]) == odd["synth_linked"]["par"]
    assert unset["knob"] == []
