"""Hand-built LZ4 sequence streams (tests/lz4_synth.py) through the emulated decoder kernels: every family, for the
frames + parse4 + copy3 pipeline at each ring size and for the serial decoder, all records side by side in one batch.
Accepted cases must decode to the builder's content, rejected ones must report their status; the verdicts are
liblz4 1.9.3's (tests/golden/lz4_synth/manifest.json; the oracle is held to them in tests/test_oracle_golden.py)."""
import json
import os

import pytest

import emu_driver as E
import helpers as H
import lz4_synth as S

VARIANTS = [0 | 12 << 4, 0 | 13 << 4, 0 | 14 << 4, 1]

with open(os.path.join(H.GOLDEN_DIR, "lz4_synth", "manifest.json")) as _f:
    MAN = json.load(_f)


@pytest.fixture(scope="module")
def cases():
    c = S.families(MAN["seed"])
    assert sorted(c) == sorted(MAN["cases"]), "the families changed: rerun tests/golden/gen_golden_lz4_synth.py"
    for name, e in c.items():
        m = MAN["cases"][name]
        assert S.sha256(e["frame"]) == m["frame_sha256"], name
        if e["status"] is not None:     # the cases built to be valid / malformed are what liblz4 says they are
            assert (e["status"] == S.ST_OK) == (m["liblz4"] == "accept"), name
    return c


def record_path(e):
    """cases the lz4-mt record path decodes: a record's capacity is its frame's content size (the host engines give a
    frame without one no output), so frames without a content size and with content go the plain .lz4 path only"""
    return (e["frame"][4] & 0x08) != 0 or e["content"] == b""


# frames without a content size that hold content: tests/test_gpu_lz4_synth.py runs them through the plain .lz4 path
PLAIN_ONLY = ["bd5_nocsize", "bd6_nocsize", "bd7_nocsize", "nocsize", "nocsize_nocheck"]


def expected(name, e):
    """(status, content or None) every decoder variant must report"""
    m = MAN["cases"][name]
    if m["liblz4"] == "accept":
        return S.ST_OK, m["content_sha256"]
    return (e["status"] if e["status"] is not None else S.ST_BAD_BLOCK), None


@pytest.mark.parametrize("variant", VARIANTS)
def test_emu_synth_families(cases, variant):
    names = [n for n in sorted(cases) if record_path(cases[n])]
    assert sorted(set(cases) - set(names)) == PLAIN_ONLY      # all others run here
    stream = b"".join(S.record(cases[n]["frame"]) for n in names)
    out, status, out_off, out_len = E.decompress(stream, variant, layout=True)
    bad = []
    for i, n in enumerate(names):
        st, sha = expected(n, cases[n])
        got = int(status[i])
        if got != st:
            bad.append((n, "status", got, st))
        elif sha is not None:
            o = int(out_off[i])
            if H.sha256(out[o:o + int(out_len[i])]) != sha:
                bad.append((n, "content"))
    assert not bad, bad


def test_emu_synth_each_record_alone(cases):
    """the same verdicts when every record is its own batch (no neighbour shares the block table or the scratch)"""
    for n in sorted(cases):
        if not record_path(cases[n]) or not n.startswith(("eob_", "stored_", "bad_", "off_65535", "lap_16384_0", "batch_")):
            continue
        st, sha = expected(n, cases[n])
        for v in (0, 1):
            out, status = E.decompress(S.record(cases[n]["frame"]), v)
            assert int(status[0]) == st, (n, v, int(status[0]))
            if sha is not None:
                assert H.sha256(out) == sha, (n, v)
