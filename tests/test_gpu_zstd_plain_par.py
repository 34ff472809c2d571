"""The block-parallel execute stage, on the device: the cases of tests/test_emu_zstd_plain_par.py through
Engine.zstd_decompress_blocks_par against Engine.zstd_decompress_blocks (committed streams at every 4th cut plus the first
and the last, every hand-built frame at every cut, 256 damaged positions)."""
import pytest

import zstd_par as R  # noqa: F401
from test_emu_zstd_plain_par import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_committed_streams_at_every_cut, test_the_decoder_reported_both_kinds_of_run, test_hand_built_frames_at_every_cut, test_dense_block_moves_the_split,
    test_history_edge, test_output_one_byte_short, test_damaged_block_in_the_middle, test_two_runs_on_two_carry_slots,
    test_damaged_committed_stream, test_switch_off_is_the_pre_call)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def par(eng):
    return eng.zstd_decompress_blocks_par


@pytest.fixture(scope="module")
def par_off(eng):
    def dec(*a, **k):
        assert eng.set_variant("zstd_run_par", 0) == 1
        try:
            return eng.zstd_decompress_blocks_par(*a, **k)
        finally:
            assert eng.set_variant("zstd_run_par", 1) == 0
    return dec


@pytest.fixture(scope="module")
def pre(eng):
    return eng.zstd_decompress_blocks_pre


@pytest.fixture(scope="module")
def serial(eng):
    return eng.zstd_decompress_blocks


@pytest.fixture(scope="module")
def kind():
    return "gpu"


def test_switch_refuses_other_values(eng):
    assert eng.set_variant("zstd_run_par", 2) == -1 and eng.set_variant("zstd_run_par", -1) == -1
    assert eng.set_variant("zstd_run_par", 1) == 1
