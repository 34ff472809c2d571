"""The span index and gpumt_brotli_decompress_batch_par on the device: the cases of tests/test_emu_brotli_rec_par.py
through Engine.brotli_compress(index=True) and Engine.brotli_decompress_par against Engine.brotli_decompress, plus the
switches of gpumt_set_variant and the bytes helper."""
import functools
import os

import pytest

import brotli_rec as R
from test_emu_brotli_rec_par import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_own_text, test_own_kinds, test_several_records_and_a_short_last_one, test_one_block_and_empty_records_have_no_index,
    test_foreign_streams, test_tampered_indexes, test_capacity_below_the_sum, test_window_record_with_a_hand_made_index,
    test_mixed_batch, test_scratch_refused, test_switch_off)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import zstdmt_amd as z
    old = os.environ.get("GPUMT_TRACE")
    os.environ["GPUMT_TRACE"] = "1"         # read when the handle is opened: the trace line carries the counts
    try:
        e = z.Engine(0)
    finally:
        if old is None:
            del os.environ["GPUMT_TRACE"]
        else:
            os.environ["GPUMT_TRACE"] = old
    yield R.Device(e)
    e.close()


@pytest.fixture(scope="module")
def serial(dev):
    return dev.serial


@pytest.fixture(scope="module")
def par(dev):
    return dev.par


@pytest.fixture(scope="module")
def encode(dev):
    return functools.lru_cache(maxsize=None)(dev.encode)


def test_both_record_decoders_behind_the_span_stage(dev, encode):
    """the record pass by dec4 first (the big-batch rule) and by the general kernel alone"""
    from test_emu_brotli_rec_par import _mixed
    b = R.Batch(_mixed(encode)[0])
    for variant in (2, 1):
        old = dev.eng.set_variant("brotli_dec", variant)
        try:
            _, got = R.check(b, dev.serial, dev.par)
        finally:
            dev.eng.set_variant("brotli_dec", old)
        assert got.stats["kept"] >= 4


def test_switches_refuse_other_values(dev):
    e = dev.eng
    assert e.set_variant("brotli_rec_par", 2) == -1 and e.set_variant("brotli_rec_par", -1) == -1
    assert e.set_variant("brotli_rec_par", 1) == 1
    assert e.set_variant("brotli_rec_min_spans", 1) == -1 and e.set_variant("brotli_rec_min_spans", 65537) == -1
    assert e.set_variant("brotli_rec_min_spans", 2) == 2
    assert e.set_variant("brotli_rec_cap_mb", -1) == -1 and e.set_variant("brotli_rec_cap_mb", 0) == 0


def test_bytes_helper(dev):
    import emu_driver as E
    data = R.kinds()["alternating"]
    stream, _, _ = dev.eng.compress_bytes(data, 1 << 20, codec="brotli", level=5, index=True)
    ro, rl, cap = E.walk_brotli_records(stream)
    recs, status, out_len, rec_par = dev.eng.brotli_decompress_par_bytes(stream, ro, rl, cap)
    assert b"".join(recs) == data and list(status) == [0] and list(out_len) == [len(data)] and list(rec_par) == [1]
    recs, status, _, rec_par = dev.eng.brotli_decompress_par_bytes(stream, ro, rl, cap, par=False)
    assert b"".join(recs) == data and list(status) == [0] and list(rec_par) == [0]
