"""The segment-parallel chain build on the device through Engine: gpumt_win_chain_plane against the Python model at seg_log
0, 12 and 16, back to back on one engine so that a call meets the head tables of the one before; both window encoders byte
for byte with "win_chain_par" 12 and 0, alone and inside a batch; refused head tables; rejected variant values."""
import pytest

import win_chain as W
from golden import cases

pytestmark = pytest.mark.gpu

SHAPES = W.shapes()
MODEL = {}
CODECS = {"zstd_L10": ("zstd", 10), "zstd_L19": ("zstd", 19), "brotli_Q9": ("brotli", 9), "brotli_Q11": ("brotli", 11)}


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


def model(name):
    if name not in MODEL:
        MODEL[name] = W.model_plane(*SHAPES[name])
    return MODEL[name]


def same(got, want, what):
    assert len(got) == len(want) and (got == want).all(), (what, [(p, int(got[p]), int(want[p]))
                                                                  for p in range(len(want)) if got[p] != want[p]][:5])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plane_is_the_models(eng, name):
    data, chunk = SHAPES[name]
    for seg_log in (0, 12, 16):
        same(eng.win_chain_plane(data, chunk, seg_log), model(name), (name, seg_log))


def test_a_call_meets_the_head_tables_of_the_one_before(eng):
    """two inputs of the same shape back to back, twice: the segment kernel resets what the carry of the call before left"""
    a, b = cases.text(300 * W.K, 91), cases.rep(cases.rnd(3000, 92), 300 * W.K)
    want = [W.model_plane(d, 100003) for d in (a, b)]
    for seg_log in (12, 16, 12):
        for d, w in ((a, want[0]), (b, want[1]), (a, want[0])):
            same(eng.win_chain_plane(d, 100003, seg_log), w, seg_log)


def records(eng, codec, data, chunk, level):
    st, ro, rl = eng.compress_bytes(data, chunk, codec=codec, level=level, win=True)
    return [st[int(ro[i]):int(ro[i]) + int(rl[i])] for i in range(len(rl))]


@pytest.mark.parametrize("codec", sorted(CODECS))
def test_records_are_the_same_with_the_variant(eng, codec):
    kind, level = CODECS[codec]
    for name in sorted(SHAPES):
        data, chunk = SHAPES[name]
        off = records(eng, kind, data, chunk, level)
        assert eng.set_variant("win_chain_par", 12) == 0
        try:
            on = records(eng, kind, data, chunk, level)
        finally:
            assert eng.set_variant("win_chain_par", 0) == 12
        assert on == off, name


@pytest.mark.parametrize("codec", ("zstd_L10", "brotli_Q9"))
def test_a_record_is_the_same_alone_and_inside_a_batch(eng, codec):
    kind, level = CODECS[codec]
    chunk = 100003
    parts = [cases.text(chunk, 41), cases.rnd(chunk // 2, 43) * 2 + b"x", cases.text(chunk, 41), cases.text(chunk - 7, 44)]
    assert eng.set_variant("win_chain_par", 12) == 0
    try:
        recs = records(eng, kind, b"".join(parts), chunk, level)
        assert len(recs) == 4 and recs[0] == recs[2]
        for k, part in enumerate(parts):
            assert records(eng, kind, part, chunk, level) == [recs[k]], k
    finally:
        assert eng.set_variant("win_chain_par", 0) == 12
    assert records(eng, kind, b"".join(parts), chunk, level) == recs


def test_refused_head_tables(eng):
    import zstdmt_amd as z
    data, chunk = SHAPES["zeros_300k"]
    assert eng.win_chain_par_scratch(len(data), chunk, 12) == 75 * (4 << 15) > 1 << 20
    off = {c: records(eng, k, data, chunk, lv) for c, (k, lv) in CODECS.items()}
    assert eng.set_variant("win_chain_cap_mb", 1) == 0 and eng.set_variant("win_chain_par", 12) == 0
    try:
        with pytest.raises(z.NativeError, match="-4"):
            eng.win_chain_plane(data, chunk, 12)
        same(eng.win_chain_plane(data, chunk, 0), model("zeros_300k"), "serial under the cap")
        for c, (k, lv) in CODECS.items():
            assert records(eng, k, data, chunk, lv) == off[c], c
    finally:
        assert eng.set_variant("win_chain_cap_mb", 0) == 1
    try:
        same(eng.win_chain_plane(data, chunk, 12), model("zeros_300k"), "the cap lifted")
        for c, (k, lv) in CODECS.items():
            assert records(eng, k, data, chunk, lv) == off[c], c
    finally:
        assert eng.set_variant("win_chain_par", 0) == 12


def test_rejected_values_leave_the_setting_alone(eng):
    import zstdmt_amd as z
    assert eng.set_variant("win_chain_par", 16) == 0
    try:
        for v in (-1, 2, 11, 25, 1 << 20):
            assert eng.set_variant("win_chain_par", v) == -1
        assert eng.set_variant("win_chain_par", 1) == 16 and eng.set_variant("win_chain_par", 24) == 1
        assert eng.set_variant("win_chain_cap_mb", -1) == -1 and eng.set_variant("win_chain_cap_mb", 0) == 0
    finally:
        assert eng.set_variant("win_chain_par", 0) == 24
    data, chunk = SHAPES["one_chunk_8192"]
    for seg_log in (-1, 1, 11, 25):
        with pytest.raises(z.NativeError, match="-3"):
            eng.win_chain_plane(data, chunk, seg_log)
    assert eng.win_chain_par_scratch(8192, 1 << 20, 12) == 2 * (4 << 12) and eng.win_chain_par_scratch(8192, 1 << 20, 13) == 0
