"""gpumt_brotli_compress_batch_win on the device through Engine: the shape list of tests/zstd_win.py at qualities 9-11, the
far repeat and the WBITS it needs, the distance cap at the edge of WBITS 24, the bar against the table encoder,
batch-position determinism, soups, qualities 0-8, the scratch-refusal fallback and the depth override.  Every stream is
decoded by both device decoders, the oracle, libbrotli and the reference build where they travelled."""
import pytest

import brotli_win as W
import emu_driver as E
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
    st, ro, rl = eng.compress_bytes(data, chunk, codec="brotli", level=level, win=win)
    return st, [st[int(ro[i]):int(ro[i]) + int(rl[i])] for i in range(len(rl))]


def check(eng, st, data):
    ro, rl, cap = E.walk_brotli_records(st)
    for variant in (2, 1):                                         # dec4 first / the general kernel alone
        old = eng.set_variant("brotli_dec", variant)
        try:
            recs, status = eng.brotli_decompress_bytes(st, ro, rl, cap)
        finally:
            eng.set_variant("brotli_dec", old)
        assert (status == 0).all() and b"".join(recs) == data, variant
    W.decode_all(st, data, emu=False)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_decompress_identical(eng, name):
    data, chunk = SHAPES[name]
    for level in W.QUALITIES:
        st, _ = records(eng, data, chunk, level)
        check(eng, st, data)
        if name in ("zeros_300k", "period_300"):
            assert len(st) < len(data) // 100
        if name == "empty":
            assert st[16:] == b"\x33"
        if name == "text_300k":
            assert W.wbits_of(st) == 19


def test_soups_at_random_qualities(eng):
    for name in sorted(SOUPS):
        data, chunk, rng = SOUPS[name]
        st, _ = records(eng, data, chunk, rng.choice(W.QUALITIES))
        check(eng, st, data)


def test_a_match_never_takes_its_source_from_the_neighbour_chunk(eng):
    import helpers as H
    data, chunk = SHAPES["chunk_1024"]
    _, recs = records(eng, data, chunk, 11)
    assert len(recs) == 300
    for k in (0, 1, 2, 150, 299):
        assert H.oracle_brotlimt_decompress(recs[k], chunk + 64) == data[k * chunk:(k + 1) * chunk]


def test_far_repeat_is_found_and_declares_its_window(eng):
    st, _ = records(eng, W.FAR, 1 << 20, 9)
    tab, _ = records(eng, W.FAR, 1 << 20, 9, win=False)
    print("far repeat: %d bytes, table encoder %d" % (len(st), len(tab)))
    # the chunk is 524288 bytes long and 2^19 - 16 < 524287, so the rule gives WBITS 20: "1" then 3 in three bits
    assert W.wbits_of(st) == 20 and st[16] & 15 == 7 and W.wbits_of(tab) == 18
    check(eng, st, W.FAR)
    assert len(st) <= W.FAR_BOUND


def test_far_repeat_under_wbits_19(eng):
    data = cases.rnd(262136, 9) * 2 + b"!"                         # the longest chunk WBITS 19 holds: 2^19 - 15 bytes
    st, _ = records(eng, data, 1 << 20, 9)
    assert W.wbits_of(st) == 19 and st[16] & 15 == 5
    check(eng, st, data)
    assert len(st) <= 262136 + 8 * W.K


@pytest.mark.parametrize("n,wbits", [(262129, 18), (262130, 19)])
def test_wbits_is_the_smallest_that_holds_the_chunk(eng, n, wbits):
    data = cases.text(n, 17)
    st, _ = records(eng, data, 1 << 20, 9)
    assert W.wbits_of(st) == wbits
    check(eng, st, data)


def test_distance_cap(eng):
    sizes = []
    for dist in (W.CAP_TAKEN, W.CAP_REFUSED):
        data = W.cap_input(dist)
        st, _ = records(eng, data, W.CAP_CHUNK, 9)
        assert W.wbits_of(st) == 24
        check(eng, st, data)
        sizes.append(len(st))
    print("distance cap: %d bytes at 2^24 - 16, %d at 2^24 - 15" % tuple(sizes))
    assert sizes[0] <= W.CAP_NOISE + 8 * W.K
    assert sizes[1] - sizes[0] >= 64 * W.K


def test_window_is_worth_having_on_text(eng):
    data = cases.text(1 << 20, 5)
    tab, _ = records(eng, data, 1 << 20, 9, win=False)
    sizes = []
    for q in W.QUALITIES:
        st, _ = records(eng, data, 1 << 20, q)
        check(eng, st, data)
        sizes.append(len(st))
    print("text 1 MiB, qualities 9 / 10 / 11: window %s, table encoder %d" % (sizes, len(tab)))
    assert sizes[0] * 1.04 < len(tab)
    assert sizes[2] <= sizes[1] <= sizes[0]
    assert [eng.brotli_win_depth(q) for q in range(12)] == [0] * 9 + [16, 32, 64]


def test_a_record_is_the_same_alone_and_inside_a_batch(eng):
    chunk = 150000
    parts = [cases.text(chunk, 41), cases.text(chunk, 42), cases.rnd(chunk // 2, 43) * 2, cases.text(chunk, 41), cases.text(chunk - 7, 44)]
    _, recs = records(eng, b"".join(parts), chunk, 10)
    assert len(recs) == 5 and recs[0] == recs[3]
    for k, part in enumerate(parts):
        assert records(eng, part, chunk, 10)[1] == [recs[k]], k


def test_qualities_below_9_are_the_table_encoder(eng):
    data = cases.text(300 * W.K, 51)
    for q in (0, 4, 8):
        assert records(eng, data, 200000, q)[0] == records(eng, data, 200000, q, win=False)[0]


def test_refused_scratch_and_depth_override(eng):
    data = cases.text(300 * W.K, 52)
    tab, _ = records(eng, data, 1 << 20, 11, win=False)
    win, _ = records(eng, data, 1 << 20, 11)
    assert len(win) < len(tab)
    assert eng.set_variant("brotli_win_cap_mb", 1) == 0
    try:
        assert records(eng, data, 1 << 20, 11)[0] == tab      # every request is above 1 MiB: the table encoder's bytes
    finally:
        assert eng.set_variant("brotli_win_cap_mb", 0) == 1
    assert records(eng, data, 1 << 20, 11)[0] == win
    assert eng.set_variant("brotli_win_depth", 257) == -1 and eng.set_variant("brotli_win_depth", -1) == -1
    assert eng.set_variant("brotli_win_depth", 64) == 0
    try:
        assert records(eng, data, 1 << 20, 9)[0] == win
        assert eng.set_variant("brotli_win_depth", 1) == 64
        d1, _ = records(eng, data, 1 << 20, 9)
    finally:
        eng.set_variant("brotli_win_depth", 0)
    assert len(d1) > len(records(eng, data, 1 << 20, 9)[0])
