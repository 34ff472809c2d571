"""The entropy pre-pass in front of the block runs, on the device: the cases of tests/test_emu_zstd_plain_pre.py through
Engine.zstd_decompress_blocks_pre against Engine.zstd_decompress_blocks."""
import pytest

import zstd_pre as P  # noqa: F401
from test_emu_zstd_plain_pre import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_equal_to_serial_and_marked, test_definer_before_the_call_stays_serial, test_several_runs_side_by_side, test_damaged_input_gets_the_serial_verdict,
    test_knob_off_marks_nothing)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pre(eng):
    return eng.zstd_decompress_blocks_pre


@pytest.fixture(scope="module")
def pre_off(eng):
    def dec(*a, **k):
        assert eng.set_variant("zstd_run_pre", 0) == 1
        try:
            return eng.zstd_decompress_blocks_pre(*a, **k)
        finally:
            assert eng.set_variant("zstd_run_pre", 1) == 0
    return dec


@pytest.fixture(scope="module")
def serial(eng):
    return eng.zstd_decompress_blocks


@pytest.fixture(scope="module")
def kind():
    return "gpu"


def test_knob_refuses_other_values(eng):
    assert eng.set_variant("zstd_run_pre", 2) == -1 and eng.set_variant("zstd_run_pre", -1) == -1
    assert eng.set_variant("zstd_run_pre", 1) == 1
