"""Hand-built zstd frames (tests/zstd_synth.py) on the device, on the four paths of tests/test_emu_zstd_synth.py:
Engine.decompress_bytes(codec="zstd") with the sequence pre-pass on and off, Engine.zstd_decompress_blocks (whole and
cut at every block boundary), Engine.zstd_decompress_blocks_pre against it, and ZSTDCB_decompressDCtx.  Verdicts:
libzstd 1.4.9's, recorded in tests/golden/zstd_synth/manifest.json, and rejection for zstd_synth.DIVERGENT; the
reference library's return code where oracle/_ref exists."""
import numpy as np
import pytest

import helpers as H
import zstd_synth as S
import zstd_synth_api as A
from test_emu_zstd_synth import (MAN, NO_FCS, API_CASES, load_cases, accepted, expected, record_path, chain_names,
                                 check_runs, check_pre, check_api, _check, _records)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return load_cases()


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("seq", [1, 0])
def test_gpu_synth_records_one_batch(eng, cases, seq):
    names = [n for n in sorted(cases) if record_path(cases[n])]
    assert sorted(set(cases) - set(names)) == NO_FCS
    recs = [S.record(cases[n]["frame"]) for n in names]
    ro = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64)
    rl = np.array([len(r) for r in recs], np.uint32)
    _, off = _records(cases, names)
    eng.set_variant("zstd_seq", seq)
    try:
        out, status = eng.decompress_bytes(b"".join(recs), ro, rl, codec="zstd")
    finally:
        eng.set_variant("zstd_seq", 1)
    bad = []
    for i, n in enumerate(names):
        _check(bad, n, expected(n, cases[n]), int(status[i]), bytes(out[int(off[i]):int(off[i + 1])]))
    assert not bad, bad


def test_gpu_synth_runs_and_cuts(eng, cases):
    bad = check_runs(cases, eng.zstd_decompress_blocks)
    assert not bad, bad


def test_gpu_synth_entropy_prepass(eng, cases):
    def off(*a, **k):
        assert eng.set_variant("zstd_run_pre", 0) == 1
        try:
            return eng.zstd_decompress_blocks_pre(*a, **k)
        finally:
            assert eng.set_variant("zstd_run_pre", 1) == 0
    bad = check_pre(cases, eng.zstd_decompress_blocks, eng.zstd_decompress_blocks_pre, off)
    assert not bad, bad


@pytest.mark.parametrize("pre", [None, "1"])
def test_gpu_synth_api(cases, pre):
    bad = check_api(cases, A.run_api("gpu", MAN["seed"], API_CASES, chain_names(cases), pre=pre))
    assert not bad, bad


@pytest.mark.skipif(not H.have_zref(), reason="reference build not present")
def test_gpu_synth_api_reference_return_codes(cases):
    """where the reference library travelled: it and this library agree on error or success for every API case the
    reference's libzstd and RFC 8878 agree on"""
    import ctypes as C
    from zstdmt_amd._native import lib_path
    lib = H.bind_lz4mt(C.CDLL(lib_path()), "ZSTDCB_")
    for n in API_CASES:
        if n in S.DIVERGENT or not record_path(cases[n]):
            continue
        st = S.record(cases[n]["frame"])
        rv, out, _, _ = H.zstdmt_decompress_via(lib, st, threads=2)
        rv_r, out_r, _, _ = H.zstdmt_decompress_via(H.zref(), st, threads=2)
        assert bool(lib.ZSTDCB_isError(rv)) == bool(H.zref().ZSTDCB_isError(rv_r)), (n, rv, rv_r)
        if not H.zref().ZSTDCB_isError(rv_r):
            assert out == out_r, n
        assert accepted(n) == (not lib.ZSTDCB_isError(rv)), n
