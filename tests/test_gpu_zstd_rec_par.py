"""Multi-block zstd-mt records through the block stages, on the device: the cases of tests/test_emu_zstd_rec_par.py
through Engine.zstd_decompress_par against Engine.zstd_decompress."""
import os

import pytest

import zstd_rec as K
from test_emu_zstd_rec_par import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_committed_records, test_committed_records_took_the_parallel_route, test_plain_frames_as_records,
    test_plain_frames_with_a_flipped_checksum_byte, test_hand_built_frames_in_one_mixed_batch, test_synth_streams_as_records,
    test_frame_level_edges, test_damaged_record, test_the_undamaged_record_takes_the_parallel_route, test_slices,
    test_default_threshold, test_switch_off, test_scratch_cap_falls_back)

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
def kind():
    return "gpu"


def test_switches_refuse_other_values(dev):
    e = dev.eng
    assert e.set_variant("zstd_rec_par", 2) == -1 and e.set_variant("zstd_rec_par", -1) == -1
    assert e.set_variant("zstd_rec_par", 1) == 1
    assert e.set_variant("zstd_rec_min_blocks", 0) == -1 and e.set_variant("zstd_rec_min_blocks", 65537) == -1
    assert e.set_variant("zstd_rec_min_blocks", 4) == 4
    assert e.set_variant("zstd_rec_slice_blocks", 1) == -1 and e.set_variant("zstd_rec_slice_blocks", 65537) == -1
    assert e.set_variant("zstd_rec_slice_blocks", 4096) == 4096
    assert e.set_variant("zstd_rec_cap_mb", -1) == -1 and e.set_variant("zstd_rec_cap_mb", 0) == 0


def test_bytes_helper(dev):
    import emu_driver as E
    from golden import cases
    data = cases.text(300 * 1024, 5)
    stream, ro, rl = dev.eng.compress_bytes(data, 1 << 20, codec="zstd")
    assert dev.eng.set_variant("zstd_rec_min_blocks", 1) == 4
    try:
        out, status, rec_par = dev.eng.zstd_decompress_par_bytes(stream, ro, rl)
    finally:
        dev.eng.set_variant("zstd_rec_min_blocks", 4)
    ro2, rl2 = E.walk_records(stream)
    assert ro2.tolist() == [0] and rl2.tolist() == [len(stream)]
    assert out == data and list(status) == [0] and list(rec_par) == [K.nblocks(stream[12:])] and rec_par[0] >= 3
