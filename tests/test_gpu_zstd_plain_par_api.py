"""tests/test_emu_zstd_plain_par_api.py's cases through the library on the device: GPUMT_ZSTD_RUN_PAR=1 and unset."""
import pytest

from test_emu_zstd_plain_par_api import (  # noqa: F401  (the same cases, with this module's `kind`)
    runs, test_same_content_trace_and_counters, test_wrong_checksum_is_refused_with_the_same_code,
    test_other_text_in_the_variable)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kind():
    return "gpu"
