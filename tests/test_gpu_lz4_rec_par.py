"""Multi-block lz4-mt records through the block stages, on the device: the cases of tests/test_emu_lz4_rec_par.py
through Engine.lz4_decompress_par against Engine.lz4_decompress."""
import os

import pytest

import lz4_rec as K
from test_emu_lz4_rec_par import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_hand_built_frames_are_the_recorded_ones, test_committed_records, test_hand_built_records_in_one_mixed_batch,
    test_frame_level_edges, test_slices, test_a_record_of_more_blocks_than_a_slice_is_a_slice_of_its_own, test_seg_route,
    test_live_streams, test_default_threshold, test_switch_off, test_scratch_cap_falls_back,
    test_interleaved_calls_on_one_stream, records_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import zstdmt_amd as z
    old = os.environ.get("GPUMT_TRACE")
    os.environ["GPUMT_TRACE"] = "1"         # read when the handle is opened: the trace line carries slices and fallback
    try:
        e = z.Engine(0)
    finally:
        if old is None:
            del os.environ["GPUMT_TRACE"]
        else:
            os.environ["GPUMT_TRACE"] = old
    yield K.Device(e)
    e.close()


@pytest.fixture(scope="module")
def serial(dev):
    return dev.serial


@pytest.fixture(scope="module")
def par(dev):
    return dev.par


@pytest.fixture(scope="module")
def compress(dev):
    def device(data, chunk, level=1):
        return dev.eng.compress_bytes(data, chunk, level=level)[0]
    return device


def test_switches_refuse_other_values(dev):
    e = dev.eng
    d = K.DEFAULT_MIN_BLOCKS
    assert e.set_variant("lz4_rec_par", 2) == -1 and e.set_variant("lz4_rec_par", -1) == -1
    assert e.set_variant("lz4_rec_par", 1) == 1
    assert e.set_variant("lz4_rec_seg", 2) == -1 and e.set_variant("lz4_rec_seg", -1) == -1
    assert e.set_variant("lz4_rec_seg", 0) == 0
    assert e.set_variant("lz4_rec_min_blocks", 1) == -1 and e.set_variant("lz4_rec_min_blocks", 65537) == -1
    assert e.set_variant("lz4_rec_min_blocks", d) == d
    assert e.set_variant("lz4_rec_slice_blocks", 1) == -1 and e.set_variant("lz4_rec_slice_blocks", 65537) == -1
    assert e.set_variant("lz4_rec_slice_blocks", 4096) == 4096
    assert e.set_variant("lz4_rec_cap_mb", -1) == -1 and e.set_variant("lz4_rec_cap_mb", 0) == 0


def test_bytes_helper(dev):
    from golden import cases
    data = cases.text(300 * 1024, 5)
    stream, ro, rl = dev.eng.compress_bytes(data, 1 << 20)
    assert dev.eng.set_variant("lz4_rec_min_blocks", 2) == K.DEFAULT_MIN_BLOCKS
    try:
        out, status, rec_par = dev.eng.lz4_decompress_par_bytes(stream, ro, rl)
    finally:
        dev.eng.set_variant("lz4_rec_min_blocks", K.DEFAULT_MIN_BLOCKS)
    assert len(records_of(stream)) == 1
    assert out == data and list(status) == [0] and list(rec_par) == [5] and K.nblocks(stream[12:]) == 5
