"""Hand-built LZ4 sequence streams (tests/lz4_synth.py) on the device: every family through Engine.decompress_bytes
for all four decoder variants in one batch, and a subset through LZ4MT_decompressDCtx, as lz4-mt records and as
the same frames in a plain .lz4 stream (no content size and BD 7 included).  Verdicts: liblz4 1.9.3's, recorded in
tests/golden/lz4_synth/manifest.json; the reference library's return code where oracle/_ref exists."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import helpers as H
import lz4_synth as S
from test_emu_lz4_synth import MAN, PLAIN_ONLY, expected, record_path

pytestmark = pytest.mark.gpu

# 0 | ring << 4 = frames + parse4 + copy3 pipeline with a 4 / 8 / 16 KiB ring, 1 = serial decoder
VARIANTS = [0 | 12 << 4, 1, 0 | 13 << 4, 0 | 14 << 4]


@pytest.fixture(scope="module")
def cases():
    c = S.families(MAN["seed"])
    assert sorted(c) == sorted(MAN["cases"])
    for name, e in c.items():
        assert S.sha256(e["frame"]) == MAN["cases"][name]["frame_sha256"], name
    return c


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lib():
    from zstdmt_amd._native import lib_path
    return H.bind_lz4mt(C.CDLL(lib_path()))


def _cap(fr):
    """the capacity the probe gives a record: its content-size field (none: 0)"""
    return struct.unpack_from("<Q", fr, 6)[0] if fr[4] & 0x08 else 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_synth_families(eng, cases, variant):
    names = [n for n in sorted(cases) if record_path(cases[n])]
    assert sorted(set(cases) - set(names)) == PLAIN_ONLY      # all others run here
    recs = [S.record(cases[n]["frame"]) for n in names]
    ro = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64)
    rl = np.array([len(r) for r in recs], np.uint32)
    oo = np.cumsum([0] + [_cap(cases[n]["frame"]) for n in names]).astype(np.uint64)
    eng.set_variant("lz4_dec", variant & 15)
    eng.set_variant("lz4_ring", (variant >> 4) or 12)
    try:
        out, status = eng.decompress_bytes(b"".join(recs), ro, rl)
    finally:
        eng.set_variant("lz4_dec", 0)
        eng.set_variant("lz4_ring", 12)
    bad = []
    for i, n in enumerate(names):
        st, sha = expected(n, cases[n])
        if int(status[i]) != st:
            bad.append((n, int(status[i]), st))
        elif sha is not None and H.sha256(out[int(oo[i]):int(oo[i + 1])]) != sha:
            bad.append((n, "content"))
    assert not bad, bad


# every frame without a content size (PLAIN_ONLY), and a subset of the rest: stored / empty blocks, header choices,
# far offsets, each malformed kind, end-of-block verdicts both ways
API_CASES = sorted(set(PLAIN_ONLY) | {
    "stored_empty_only", "stored_empty_mid", "stored_empty_endmark", "linked_prev", "short_blocks", "bd7", "bcheck",
    "dictid", "off_65535_full_block", "lap_8192_1", "batch_2048_1", "stage_pad3", "bad_offset0",
    "bad_offset_past_start_later", "bad_offset_across_indep", "bad_block_above_max", "bad_lits_past_end",
    "bad_varint_lit_off_end", "bad_varint_ml_off_end", "bad_ends_in_match", "bad_past_64k", "eob_full_last2_m8",
    "eob_full_last5_m8", "eob_full_back12_l5", "eob_short_last3_m20", "eob_short_last4_m20", "eob_full_lit15_l2"})


@pytest.mark.parametrize("name", API_CASES)
def test_api_synth_plain_and_records(lib, cases, name):
    """LZ4MT_decompressDCtx: the frame alone (plain .lz4 path), and as an lz4-mt record where the record path takes it"""
    e, m = cases[name], MAN["cases"][name]
    fr = e["frame"]
    streams = [("plain", fr)]
    if record_path(e):
        streams.append(("record", S.record(fr)))
    for kind, st in streams:
        rv, out, _, _ = H.lz4mt_decompress_via(lib, st, threads=2)
        if H.have_ref():
            rv_r, out_r, _, _ = H.lz4mt_decompress_via(H.ref(), st, threads=2)
            assert bool(lib.LZ4MT_isError(rv)) == bool(H.ref().LZ4MT_isError(rv_r)), (kind, rv, rv_r)
            if not H.ref().LZ4MT_isError(rv_r):
                assert out == out_r, kind
        if m["liblz4"] == "accept":
            assert not lib.LZ4MT_isError(rv), (kind, rv)
            assert H.sha256(out) == m["content_sha256"], kind
        else:
            assert lib.LZ4MT_isError(rv), (kind, rv)


def test_api_synth_plain_stream_of_many_frames(lib, cases):
    """every frame liblz4 accepts, back to back in one plain .lz4 stream"""
    names = [n for n in sorted(cases) if MAN["cases"][n]["liblz4"] == "accept"]
    st = b"".join(cases[n]["frame"] for n in names)
    rv, out, _, _ = H.lz4mt_decompress_via(lib, st, threads=4)
    assert rv == 0
    want = b"".join(cases[n]["content"] for n in names)
    assert [H.sha256(cases[n]["content"]) for n in names] == [MAN["cases"][n]["content_sha256"] for n in names]
    assert out == want
