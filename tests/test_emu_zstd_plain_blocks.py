"""Plain .zst input decoded run by run (zstdmt_amd/csrc/host/mt_zstd_plain.inc over gpumt_zstd_decompress_blocks and
gpumt_xxh64_carry), on the CPU: the two new kernels directly under the emulator, and the host engine over the emulated
device with 16 KiB batches, so a frame spans many batches.  tests/test_gpu_zstd_plain_blocks.py runs the same cases on
the device: the test functions below take what differs (`decode`, `xxh64`, `api`, `cli`) as fixtures."""
import os
import subprocess
import sys

import pytest

import helpers as H
import zstd_blocks as Z
from golden import cases

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def decode():
    return Z.emu_decode_blocks


@pytest.fixture(scope="module")
def xxh64():
    return Z.emu_xxh64_carry


@pytest.fixture(scope="module")
def api():
    return Z.run_api("emu")


@pytest.fixture(scope="module")
def cli():
    H.locked_make(EMU_DIR, "cli", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(EMU_DIR, "bin", "zstd-mt")


# ---- 1. every cut -----------------------------------------------------------------------------------------------------
def test_the_cut_frames_cover_every_kind_of_carried_state():
    """the small parser of the literal-type bits and the sequence-modes byte: across the frames of the next test there is
    a cut directly before a treeless-literals block and before a Repeat_Mode table of each of LL, OF and ML"""
    kinds = set()
    for name in Z.CUT_NAMES:
        info = Z.walk(Z.cut_frames()[name][0])
        kinds |= set().union(*Z.cut_kinds(info).values())
        if name.startswith("live_"):
            assert len(info["blocks"]) == 12
    assert {"treeless", "repeat_ll", "repeat_of", "repeat_ml"} <= kinds, kinds


@pytest.mark.parametrize("name", Z.CUT_NAMES)
def test_the_oracle_decodes_the_cut_frames(name):
    fr, want = Z.cut_frames()[name]
    assert H.oracle_zstdmt_decompress(H.mt_record(fr), len(want) + 64) == want


@pytest.mark.parametrize("name,cut", Z.cut_params())
def test_every_cut(decode, name, cut):
    """the frame as two runs, split at a block boundary -- each of them in turn --, the first run's output as the second
    one's history"""
    fr, want = Z.cut_frames()[name]
    info = Z.walk(fr)
    assert cut < len(info["blocks"])
    out, st = Z.decode_cut(decode, info, cut)
    assert st == [0, 0] and out == want


def _hand_frame():
    a, b = cases.text(3000, 71), cases.rnd(700, 72)
    lits = cases.text(20, 73)
    blocks = [("raw", a), ("rle", 0x41, 500), ("raw", b), ("cooked", Z.match_block(lits, 4100, 30)), ("raw", b"")]
    plain = a + b"\x41" * 500 + b + lits
    plain += plain[len(plain) - 4100:len(plain) - 4100 + 30]
    return Z.frame_of(blocks, csize=len(plain)), plain


def test_cuts_before_raw_rle_and_empty_last_blocks(decode):
    fr, want = _hand_frame()
    assert H.oracle_zstdmt_decompress(H.mt_record(fr), len(want) + 64) == want
    info = Z.walk(fr)
    seen = set()
    for cut, kinds in Z.cut_kinds(info).items():
        out, st = Z.decode_cut(decode, info, cut)
        assert st == [0, 0] and out == want, cut
        seen |= kinds
    assert {"raw", "rle", "empty"} <= seen


# ---- 2. history -------------------------------------------------------------------------------------------------------
def test_match_into_the_history_and_one_byte_in_front_of_it(decode):
    hist, lits = cases.text(1000, 74), cases.text(20, 75)
    info = Z.walk(Z.frame_of([("raw", hist), ("cooked", Z.match_block(lits, 1020, 30))]))
    s1, b1, r1, o1 = Z.tables(info, 0, 1)
    out1, rl1, st1, cy = decode(s1, b1, r1, o1)
    assert list(st1) == [0] and out1[:1000] == hist
    # the match source is the first byte of the history
    s2, b2, r2, o2 = Z.tables(info, 1, 2, hist=1000)
    out2, rl2, st2, _ = decode(s2, b2, r2, o2, history=hist, carry=cy)
    assert list(st2) == [0] and int(rl2[0]) == 50 and out2[1000:1050] == lits + hist[:30]
    # one byte of history less: the same match starts in front of it; nothing but the history is in the output area
    s3, b3, r3, o3 = Z.tables(info, 1, 2, hist=999)
    out3, rl3, st3, _ = decode(s3, b3, r3, o3, history=hist[1:], carry=cy)
    assert list(st3) == [Z.ST_BAD_BLOCK]
    assert out3[:999] == hist[1:] and out3[999:] == b"\xCC" * (o3 - 999)


def test_treeless_block_at_the_start_of_a_frame(decode):
    info = Z.walk(Z.fixture("l3_plain")[0])
    k = next(c for c, kinds in Z.cut_kinds(info).items() if "treeless" in kinds)
    s, b, r, o = Z.tables(info, k, k + 1)
    r["flags"] = Z.ZRUN_FIRST | Z.ZRUN_LAST
    _, _, st, _ = decode(s, b, r, o)
    assert list(st) == [Z.ST_BAD_BLOCK]
    # and behind a carry that holds no table (the run before it was a raw block)
    raw = Z.walk(Z.frame_of([("raw", b"0123456789"), ("raw", b"")]))
    s1, b1, r1, o1 = Z.tables(raw, 0, 1)
    _, _, st1, cy = decode(s1, b1, r1, o1)
    r["flags"] = Z.ZRUN_LAST
    _, _, st, _ = decode(s, b, r, o, carry=cy)
    assert list(st1) == [0] and list(st) == [Z.ST_BAD_BLOCK]


def test_table_entries_that_leave_the_buffers(decode):
    info = Z.walk(_hand_frame()[0])
    s, b, r, o = Z.tables(info, 0, 3)
    for field, val, arr in (("src_off", len(s) + 1, "b"), ("src_len", len(s) + 1, "b"), ("out_off", o + 1, "r"),
                            ("out_cap", o + 1, "r"), ("first", 4, "r"), ("count", 4, "r"), ("hist", 1, "r"),
                            ("carry", 2, "r"), ("block_max", 131073, "b")):
        bb, rr = b.copy(), r.copy()
        (bb if arr == "b" else rr)[field][0] = val
        out, rl, st, _ = decode(s, bb, rr, o)
        assert int(st[0]) == 1 and out == b"\xCC" * o, field


# ---- 3. the carried checksum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 100, 4096, 70001])
def test_xxh64_carried_state(xxh64, n):
    data = cases.rnd(n, n + 5)
    want = Z.xxh64_low32(data)
    splits = [[n], [0, n], [n, 0], [n // 2, n - n // 2], [min(n, 1), max(n - 1, 0)], [min(n, 31), max(n - 31, 0)],
              [min(n, 32), max(n - 32, 0)], [min(n, 33), max(n - 33, 0)]]
    if n >= 100:
        splits += [[5, 7, 4, 16, 32, n - 64], [1] * 40 + [n - 40], [31, 1, 33, 0, n - 65]]
    for pieces in splits:
        assert xxh64(data, pieces) == want, pieces


# ---- 4. through ZSTDCB_decompressDCtx, 16 KiB batches -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["checksum", "no_content_size", "level19_window", "frame_skippable_frame"])
def test_one_frame_over_many_batches(api, name):
    import hashlib
    st, want = Z.api_cases()[name]
    r = api[name]
    assert r["rv"] == 0 and r["nout"] == len(want) and r["sha"] == hashlib.sha256(want).hexdigest()
    assert r["stats"] == [0, len(st), len(want)]
    assert r["max_write"] <= 131072
    assert r["batches"] >= 3, r.get("trace")
    if name == "level19_window":
        assert Z.walk(st)["window"] > 4 * 16384          # the window is larger than a batch's output
    if H.have_zref():
        rv_r, out_r, io_r, stats_r = H.zstdmt_decompress_via(H.zref(), st, threads=2)
        assert rv_r == 0 and out_r == want and list(stats_r) == r["stats"]
        assert [list(x) for x in io_r.reads[:2]] == r["reads"][:2]     # the sniff, then the rest of the first buffer


# ---- 5. errors after the first batch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["err_flip_third_batch", "err_cut_in_later_block", "err_cut_in_checksum",
                                  "err_wrong_content_size", "err_wrong_checksum", "err_garbage_after"])
def test_errors_after_the_first_batch(api, name):
    assert api[name]["rv"] == Z.ERR(Z.E_LIB), api[name]
    if name == "err_flip_third_batch":
        assert api[name]["batches"] >= 3 and api[name]["nout"] > 0       # the first two batches were written


# ---- the command line tool --------------------------------------------------------------------------------------------
def test_cli_decodes_a_committed_stream_under_small_batches(cli):
    fr, want = Z.fixture("l19_chk_size")
    env = dict(os.environ, GPUMT_BATCH_KB="16", GPUMT_TRACE="1")
    p = subprocess.run([cli, "-d", "-c"], input=fr, capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-300:]
    assert p.stdout == want
    assert b"[zstdmt plain]" in p.stderr


def test_new_kernels_under_the_strict_emulator():
    env = dict(os.environ, EMU_STRICT="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "(every_cut and (l19_tiled or l3_chk_size)) or raw_rle or history or treeless or table_entries or xxh64_carried"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-1500:]
