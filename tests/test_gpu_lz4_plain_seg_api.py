"""tests/test_emu_lz4_plain_seg_api.py's cases through the library on the device: GPUMT_LZ4_BLOCK_SEG=1 and unset."""
import pytest

import lz4_blocks as B
import lz4_seg_api as A

pytestmark = pytest.mark.gpu

NAMES = sorted(A.api_cases())


@pytest.fixture(scope="module")
def on():
    return A.run_api("gpu", "1")


@pytest.fixture(scope="module")
def off():
    return A.run_api("gpu", None)


@pytest.mark.parametrize("name", NAMES)
def test_same_bytes_callbacks_counters_and_error_on_and_off(on, off, name):
    A.check_on_off(on, off, name, B.ERR(B.E_LIB))
