"""Hand-built zstd frames (tests/zstd_synth.py) through the emulated decoder kernels, on every path a frame is eligible
for: the record decoder (E.zstd_decompress, sequence pre-pass on and off, all records in one batch and a subset alone),
the run decoder (one run, and cut at every block boundary with carry and history), the entropy pre-pass in front of it
(on and off against the serial call) and ZSTDCB_decompressDCtx.  Accepted cases must decode to the recorded content,
rejected ones report their status.  The verdicts are libzstd 1.4.9's (tests/golden/zstd_synth/manifest.json) except for
the cases of zstd_synth.DIVERGENT, which RFC 8878 forbids and libzstd accepts: those must be rejected."""
import json
import os

import numpy as np
import pytest

import emu_driver as E
import helpers as H
import zstd_blocks as Z
import zstd_pre as P
import zstd_synth as S
import zstd_synth_api as A

with open(os.path.join(H.GOLDEN_DIR, "zstd_synth", "manifest.json")) as _f:
    MAN = json.load(_f)


def load_cases():
    c = S.families(MAN["seed"])
    assert sorted(c) == sorted(MAN["cases"]), "the families changed: rerun tests/golden/gen_golden_zstd_synth.py"
    for name, e in c.items():
        m = MAN["cases"][name]
        assert S.sha256(e["frame"]) == m["frame_sha256"], name
        if m["libzstd"] == "accept" and name not in S.DIVERGENT:
            assert S.sha256(e["content"]) == m["content_sha256"], name
        if e["status"] is not None:     # built valid / malformed is what libzstd says, but for the named divergences
            assert ((e["status"] == S.ST_OK) == (m["libzstd"] == "accept")) != (name in S.DIVERGENT), name
    assert all(MAN["cases"][n]["libzstd"] == "accept" and c[n]["status"] not in (None, S.ST_OK) for n in S.DIVERGENT)
    return c


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def accepted(name):
    return MAN["cases"][name]["libzstd"] == "accept" and name not in S.DIVERGENT


def expected(name, e):
    """(status, content sha or None) of the whole frame; status None = any status but 0"""
    if accepted(name):
        return S.ST_OK, MAN["cases"][name]["content_sha256"]
    return e["status"], None


def expected_blocks(name, e):
    """the same for the paths that are given the blocks and not the frame around them: what is wrong with a frame's
    header, content size or checksum does not reach them"""
    if not accepted(name) and e["level"] == "frame":
        return S.ST_OK, S.sha256(e["content"])
    return expected(name, e)


def record_path(e):
    """the record decoder sizes a record's output by its Frame_Content_Size field"""
    return S.has_fcs(e["frame"])


def walkable(e):
    """the block-table paths need a frame whose headers zstd_blocks.walk can follow to the last block"""
    try:
        info = Z.walk(e["frame"])
    except (IndexError, AssertionError):
        return False
    return all(b["type"] != 3 and len(b["raw"]) == 3 + (1 if b["type"] == 1 else int.from_bytes(b["raw"][:3], "little") >> 3)
               for b in info["blocks"])


# frames without a Frame_Content_Size field: the run decoder and the API take them, the record decoder does not
NO_FCS = ["hdr_checksum_nofcs", "hdr_empty_frame_nofcs", "hdr_fcs0", "off_beyond_window", "window_1k_block_at",
          "window_1k_block_over", "window_1k_raw_over"]
# frames with a block whose header cannot be followed: a reserved block type, a Compressed_Block without a byte
NOT_WALKABLE = ["hdr_block_type3", "hdr_block_type3_later", "hdr_comp_block_size_0"]
# a match that reaches beyond the Window_Size into content the frame did produce (the builder's "far" list): libzstd's
# one-shot call and a decoder that has the whole frame at hand take it; one that keeps a window of history between two
# calls (RFC 8878 3.1.1.1.2: what a decoder must keep) has to refuse it when the source is not in what it kept
BEYOND_WINDOW = ["off_beyond_window"]
# a Window_Size of 3.75 GiB: the record decoder sizes by the content size and decodes it, the streaming API refuses such a
# window as the reference's ZSTD_decompressStream does (above 2^27)
HUGE_WINDOW = ["hdr_window_e21_m7"]


def source_kept(e, n1, hist):
    """a second call that starts at output position n1 with `hist` bytes of history holds the source of every far match"""
    return all(p < n1 or p - o >= n1 - hist for p, o in e["far"])


def chain_names(cases):
    """every accepted frame the streaming API takes (a far match inside one small frame stays inside one batch)"""
    assert HUGE_WINDOW == sorted(n for n, e in cases.items() if not e["frame"][4] & 0x20 and e["frame"][5] >> 3 > 17)
    assert BEYOND_WINDOW == sorted(n for n, e in cases.items() if e["far"])
    return [n for n in sorted(cases) if accepted(n) and n not in HUGE_WINDOW]


# every record alone as well: what depends on the neighbours in a batch (scratch slots, the look-ahead, hand-off)
ALONE = ("sp_", "nseq_", "tab_small_then_general", "tab_al_9_8_9", "unit_", "ml_1310", "huf_bad_", "seq_bad_", "rep_rep0")
API_CASES = ["batch_129", "hdr_window_e21_m7", "off_beyond_window", "sp_nseq_0x7F00", "sp_rep_run_3_new", "hdr_checksum", "hdr_checksum_nofcs", "hdr_checksum_wrong", "hdr_empty_frame", "huf4_16384",
             "huf_bad_jump_overrun", "huf_treeless_after_raw_rle", "nseq_above_seqcap", "off_code19_rle_history",
             "off_position_plus1_block2", "rep_across_blocks", "rep_rep0_minus1_zero", "seq_bad_one_bit_short",
             "tab_small_then_general", "unit_17_followers", "unit_regen_128k_over", "window_1k_block_at"]


def _check(bad, name, want, got_status, got_bytes):
    st, sha = want
    if (got_status != st) if st is not None else (got_status == 0):
        bad.append((name, "status", got_status, st))
    elif sha is not None and S.sha256(got_bytes) != sha:
        bad.append((name, "content", len(got_bytes)))


def _records(cases, names):
    stream = b"".join(S.record(cases[n]["frame"]) for n in names)
    caps = []
    for n in names:
        c = S.content_size_field(cases[n]["frame"])
        ok = c is not None and c <= 0x7FFFFFFF and not cases[n]["frame"][4] & 8
        caps.append(c if ok else 0)
    return stream, np.cumsum([0] + caps)


@pytest.mark.parametrize("seq_off", [False, True])
def test_emu_synth_records_one_batch(cases, seq_off):
    names = [n for n in sorted(cases) if record_path(cases[n])]
    assert sorted(set(cases) - set(names)) == NO_FCS
    stream, off = _records(cases, names)
    if seq_off:
        os.environ["EMU_ZSTD_SEQ"] = "1"
    try:
        out, status = E.zstd_decompress(stream)
        marks = E.zstd_last_marks()
    finally:
        os.environ.pop("EMU_ZSTD_SEQ", None)
    # the sequence pre-pass took blocks when it was on (every sp_ frame has two for it), none when it was off
    assert marks == 0 if seq_off else marks >= 2 * sum(n.startswith("sp_") and accepted(n) for n in names) > 0
    bad = []
    for i, n in enumerate(names):
        _check(bad, n, expected(n, cases[n]), int(status[i]), out[off[i]:off[i + 1]])
    assert not bad, bad


def test_emu_synth_each_record_alone(cases):
    names = [n for n in sorted(cases) if record_path(cases[n]) and n.startswith(ALONE)]
    assert len(names) > 30
    bad = []
    for n in names:
        out, status = E.zstd_decompress(S.record(cases[n]["frame"]))
        _check(bad, n, expected(n, cases[n]), int(status[0]), out)
        if n.startswith("sp_") and E.zstd_last_marks() < 2:
            bad.append((n, "the sequence pre-pass did not take the frame"))
    assert not bad, bad


def run_names(cases):
    names = [n for n in sorted(cases) if walkable(cases[n])]
    assert sorted(set(cases) - set(names)) == NOT_WALKABLE and set(BEYOND_WINDOW) <= set(names)
    return names


def check_runs(cases, decode):
    """every walkable frame as one run, and cut in two at every block boundary (carry and history as the host engine
    hands them on): the same bytes, length and verdict at every cut"""
    bad = []
    for n in run_names(cases):
        info = Z.walk(cases[n]["frame"])
        s, b, r, o = Z.tables(info, 0, len(info["blocks"]))
        out, rl, st, _ = decode(s, b, r, o)
        whole = (int(st[0]), out[:int(rl[0])])
        _check(bad, n, expected_blocks(n, cases[n]), *whole)
        for cut in range(1, len(info["blocks"])):
            got, sts = Z.decode_cut(decode, info, cut)
            n1 = sum(b["cap"] for b in info["blocks"][:cut])
            if not source_kept(cases[n], n1, min(n1, info["window"])):
                # the second call does not hold the source: refused there, what was decoded before it stands
                if sts[0] != 0 or not sts[1] or len(got) < n1 or got != whole[1][:len(got)]:
                    bad.append((n, "cut beyond the kept window", cut, sts, len(got)))
                continue
            verdict = next((x for x in sts if x), 0)
            if verdict != whole[0] or (verdict == 0 and got != whole[1]) or (verdict and got != whole[1][:len(got)]):
                bad.append((n, "cut", cut, sts, len(got), len(whole[1])))
    return bad


def test_emu_synth_runs_and_cuts(cases):
    bad = check_runs(cases, Z.emu_decode_blocks)
    assert not bad, bad


def check_pre(cases, serial, pre, pre_off):
    """the entropy pre-pass on and off give what the serial call gives: bytes, run length, status, carry"""
    bad = []
    for n in run_names(cases):
        info = Z.walk(cases[n]["frame"])
        nb = len(info["blocks"])
        # as one call; frames of at most 64 KiB also as two calls with the boundary in the middle (carry compared)
        for cut in sorted({0, nb // 2 if len(cases[n]["content"] or b"") <= 65536 else 0}):
            want = P.decode_parts(serial, info, cut)
            for kind, dec in (("on", pre), ("off", pre_off)):
                got = P.decode_parts(dec, info, cut)
                if [g[:4] for g in got] != [w[:4] for w in want]:
                    bad.append((n, kind, cut, [g[1:3] for g in got], [w[1:3] for w in want]))
                if kind == "off" and any(m for g in got for m in g[4]):
                    bad.append((n, "marks with the pre-pass off"))
                if kind == "on":
                    bounds = [(0, nb)] if cut == 0 else [(0, cut), (cut, nb)]
                    for g, (lo, hi) in zip(got, bounds):
                        if g[2] == 0 and g[4] != P.expected_marks(info, lo, hi):
                            bad.append((n, "marks", cut, lo, g[4], P.expected_marks(info, lo, hi)))
    return bad


def test_emu_synth_entropy_prepass(cases):
    off = lambda *a, **k: P.emu_decode_blocks_pre(*a, pre_on=0, **k)  # noqa: E731
    bad = check_pre(cases, Z.emu_decode_blocks, P.emu_decode_blocks_pre, off)
    assert not bad, bad


def check_api(cases, res):
    bad = []
    for n in API_CASES:
        e = cases[n]
        for kind in ("plain", "record"):
            r = res.get("%s/%s" % (n, kind))
            if r is None:
                assert kind == "record" and not record_path(e)
                continue
            if accepted(n) and not (n in HUGE_WINDOW and kind == "plain"):
                if r["err"] or r["sha"] != MAN["cases"][n]["content_sha256"]:
                    bad.append((n, kind, r["rv"], r["nout"]))
            elif not r["err"]:
                bad.append((n, kind, "accepted"))
    chain = chain_names(cases)
    r = res["chain/plain"]
    if r["err"] or r["sha"] != S.sha256(b"".join(cases[n]["content"] for n in chain)):
        bad.append(("chain", r["rv"], r["nout"]))
    return bad


@pytest.mark.parametrize("pre", [None, "1"])
def test_emu_synth_api(cases, pre):
    assert set(API_CASES) <= set(cases)
    chain = chain_names(cases)
    bad = check_api(cases, A.run_api("emu", MAN["seed"], API_CASES, chain, pre=pre))
    assert not bad, bad
