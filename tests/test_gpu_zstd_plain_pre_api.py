"""The entropy pre-pass under ZSTDCB_decompressDCtx, on the device: the cases of tests/test_emu_zstd_plain_pre_api.py."""
import pytest

import zstd_pre_api as A
from test_emu_zstd_plain_pre_api import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_same_content_trace_and_counters_on_and_off, test_wrong_checksum_is_refused_with_the_same_code,
    test_batches_of_several_blocks, test_other_values_of_the_variable_are_ignored)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def on():
    return A.run_api("gpu", True)


@pytest.fixture(scope="module")
def off():
    return A.run_api("gpu", False)


@pytest.fixture(scope="module")
def wide():
    only = ["level3", "level19"]
    return (A.run_api("gpu", True, 512, only), A.run_api("gpu", False, 512, only), A.run_api("gpu", "2", 512, ["level3"]))
