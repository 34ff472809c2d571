"""gpumt_zstd_compress_batch_win on the device through Engine: the shape list of tests/zstd_win.py, the far repeat, the bar
against the table encoder, batch-position determinism, soups at random levels, levels 1-9 and the scratch-refusal fallback.
Every stream is decoded by the device, the oracle and, where it travelled, the reference build."""
import pytest

import emu_driver as E
import helpers as H
import zstd_win as W
from golden import cases

pytestmark = pytest.mark.gpu

SHAPES = W.shapes()
SOUPS = W.soups()


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


def records(eng, data, chunk, level, win=True):
    st, ro, rl = eng.compress_bytes(data, chunk, codec="zstd", level=level, win=win)
    return st, [st[int(ro[i]):int(ro[i]) + int(rl[i])] for i in range(len(rl))]


def check(eng, st, data):
    ro, rl = E.walk_records(st)
    out, status = eng.decompress_bytes(st, ro, rl, codec="zstd")
    assert (status == 0).all() and out == data
    W.decode_all(st, data, emu=False)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_decompress_identical(eng, name):
    data, chunk = SHAPES[name]
    for level in W.LEVELS:
        st, _ = records(eng, data, chunk, level)
        check(eng, st, data)
        if name in ("zeros_300k", "period_300"):
            assert len(st) < len(data) // 100


def test_soups_at_random_levels(eng):
    for name in sorted(SOUPS):
        data, chunk, rng = SOUPS[name]
        st, _ = records(eng, data, chunk, rng.randrange(10, 23))
        check(eng, st, data)


def test_far_repeat_is_found(eng):
    st, _ = records(eng, W.FAR, 1 << 20, 10)
    tab, _ = records(eng, W.FAR, 1 << 20, 10, win=False)
    print("far repeat: %d bytes, table encoder %d" % (len(st), len(tab)))
    check(eng, st, W.FAR)
    assert len(st) <= W.FAR_BOUND


def test_window_is_worth_having_on_text(eng):
    data = cases.text(4 << 20, 77)
    st, _ = records(eng, data, 1 << 20, 10)
    tab, _ = records(eng, data, 1 << 20, 10, win=False)
    print("text 4 MiB at 1 MiB chunks, level 10: window %d, table encoder %d" % (len(st), len(tab)))
    check(eng, st, data)
    assert len(st) * 1.04 < len(tab)


def test_a_record_is_the_same_alone_and_inside_a_batch(eng):
    chunk = 150000
    parts = [cases.text(chunk, 41), cases.text(chunk, 42), cases.rnd(chunk // 2, 43) * 2, cases.text(chunk, 41), cases.text(chunk - 7, 44)]
    _, recs = records(eng, b"".join(parts), chunk, 13)
    assert len(recs) == 5 and recs[0] == recs[3]
    for k, part in enumerate(parts):
        assert records(eng, part, chunk, 13)[1] == [recs[k]], k


def test_levels_below_10_are_the_table_encoder(eng):
    data = cases.text(300 * W.K, 51)
    for lv in (1, 3, 9):
        assert records(eng, data, 200000, lv)[0] == records(eng, data, 200000, lv, win=False)[0]
    assert [eng.zstd_win_depth(lv) for lv in (1, 9, 10, 12, 13, 15, 16, 18, 19, 22)] == [0, 0, 8, 8, 16, 16, 32, 32, 64, 64]


def test_refused_scratch_and_depth_override(eng):
    data = cases.text(300 * W.K, 52)
    tab, _ = records(eng, data, 1 << 20, 19, win=False)
    win, _ = records(eng, data, 1 << 20, 19)
    assert len(win) < len(tab)
    assert eng.set_variant("zstd_win_cap_mb", 1) == 0
    try:
        assert records(eng, data, 1 << 20, 19)[0] == tab      # every request is above 1 MiB: the table encoder's bytes
    finally:
        assert eng.set_variant("zstd_win_cap_mb", 0) == 1
    assert records(eng, data, 1 << 20, 19)[0] == win
    assert eng.set_variant("zstd_win_depth", 257) == -1 and eng.set_variant("zstd_win_depth", -1) == -1
    assert eng.set_variant("zstd_win_depth", 64) == 0
    try:
        assert records(eng, data, 1 << 20, 10)[0] == win
    finally:
        assert eng.set_variant("zstd_win_depth", 0) == 64
