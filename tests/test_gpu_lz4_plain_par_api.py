"""tests/test_emu_lz4_plain_par_api.py's cases through the library on the device: GPUMT_LZ4_RUN_PAR on and off."""
import pytest

import lz4_blocks as B
import lz4_par_api as A

pytestmark = pytest.mark.gpu

NAMES = sorted(A.api_cases())


@pytest.fixture(scope="module")
def on():
    return A.run_api("gpu", True)


@pytest.fixture(scope="module")
def off():
    return A.run_api("gpu", False)


@pytest.mark.parametrize("name", NAMES)
def test_same_bytes_callbacks_counters_and_error_on_and_off(on, off, name):
    A.check_on_off(on, off, name, B.ERR(B.E_LIB))


def test_other_values_of_the_variable(on):
    odd = A.run_api("gpu", "yes", only=["synth_linked"])
    for key in A.KEYS:
        assert odd["synth_linked"][key] == on["synth_linked"][key], key
    assert odd["knob"] and all("GPUMT_LZ4_RUN_PAR=yes ignored" in k for k in odd["knob"])
