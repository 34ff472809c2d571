"""gpumt_brotli_compress_batch_win under the emulator: every stream through the oracle, both emulated decoder kernels and
libbrotli, records that decode alone, the far repeat the 128 KiB window cannot reach with the WBITS it needs, the distance
cap at the edge of WBITS 24, the ratio bars between the table encoder and the qualities, determinism in the grid and in the
batch position, qualities 0-8 and the scratch-refusal fallback -- and a subset of it under the strict and the shuffled
emulator.

test_distance_cap encodes two 16 MiB + 70 KiB inputs in a 17 MiB chunk and decodes each four times: about two minutes of the
plain emulator in all (the chain build and the zero run dominate), which is why it runs under the plain emulator alone."""
import os
import subprocess
import sys

import pytest

import helpers as H
import brotli_win as W
from golden import cases

SHAPES = W.shapes()
SOUPS = W.soups()
TEXT = cases.text(1 << 20, 5)
SIZES = {}


def text_size(level, call="win"):
    """the 1 MiB text at chunk 1 MiB, once per quality and call (decoded where it is encoded)"""
    if (level, call) not in SIZES:
        st = W.emu_stream(TEXT, 1 << 20, level, grid=8, call=call)
        W.decode_all(st, TEXT, emu=level == 9)
        SIZES[(level, call)] = (len(st), st)
    return SIZES[(level, call)]


# ---- 1. decompress-identical ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", W.QUALITIES, ids=lambda q: "Q%d" % q)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_decompress_identical(name, level):
    data, chunk = SHAPES[name]
    recs, ran = W.emu_records(data, chunk, level)
    st = b"".join(recs)
    assert ran == {9: 16, 10: 32, 11: 64}[level]
    W.decode_all(st, data)
    if name in ("zeros_300k", "period_300"):
        assert len(st) < len(data) // 100
    if name == "empty":
        assert st[16:] == b"\x33"                                  # the empty stream is unchanged


@pytest.mark.parametrize("name", sorted(SOUPS))
def test_soup(name):
    data, chunk, rng = SOUPS[name]
    st = W.emu_stream(data, chunk, rng.choice(W.QUALITIES), grid=rng.choice((1, 3, 8)))
    W.decode_all(st, data)


# ---- 2. no source from the neighbour chunk -------------------------------------------------------------------------------
def test_a_match_never_takes_its_source_from_the_neighbour_chunk():
    """every record decodes on its own: chunk k's record alone gives chunk k"""
    data, chunk = SHAPES["chunk_1024"]
    recs, ran = W.emu_records(data, chunk, 11, grid=8)
    assert ran == 64 and len(recs) == 300
    for k in (0, 1, 2, 150, 299):
        assert H.oracle_brotlimt_decompress(recs[k], chunk + 64) == data[k * chunk:(k + 1) * chunk]


# ---- 3. far repeat and WBITS ---------------------------------------------------------------------------------------------
def test_far_repeat_is_found_and_declares_its_window():
    """256 KiB of noise twice in one 1 MiB chunk: the second copy lies 262144 back, beyond the 2^18 - 16 of WBITS 18, so
    the stream has to declare a larger window; the table encoder, whose matches stay in their 128 KiB block, stores both
    copies"""
    st = W.emu_stream(W.FAR, 1 << 20, 9)
    tab = W.emu_stream(W.FAR, 1 << 20, 9, call="level")
    print("far repeat: %d bytes, table encoder %d" % (len(st), len(tab)))
    # the chunk is 524288 bytes long and 2^19 - 16 < 524287, so the rule gives WBITS 20: "1" then 3 in three bits
    assert W.wbits_of(st) == 20 and st[16] & 15 == 7 and W.wbits_of(tab) == 18
    W.decode_all(st, W.FAR)
    assert len(st) <= W.FAR_BOUND


def test_far_repeat_under_wbits_19():
    """the longest chunk WBITS 19 holds, 2^19 - 15 bytes: 262136 bytes of noise twice and one byte; the copy lies beyond
    2^18 - 16"""
    data = cases.rnd(262136, 9) * 2 + b"!"
    st = W.emu_stream(data, 1 << 20, 9)
    assert len(data) - 1 == (1 << 19) - 16 and W.wbits_of(st) == 19 and st[16] & 15 == 5
    W.decode_all(st, data)
    assert len(st) <= 262136 + 8 * W.K


@pytest.mark.parametrize("n,wbits", [(262129, 18), (262130, 19)])
def test_wbits_is_the_smallest_that_holds_the_chunk(n, wbits):
    data = cases.text(n, 17)
    st = W.emu_stream(data, 1 << 20, 9)
    assert W.wbits_of(st) == wbits
    W.decode_all(st, data)


def test_wbits_of_the_text():
    data, chunk = SHAPES["text_300k"]
    assert W.wbits_of(W.emu_stream(data, chunk, 9)) == 19


# ---- 4. distance cap -----------------------------------------------------------------------------------------------------
def test_distance_cap():
    """70 KiB of noise, zeros, the noise again in one 17 MiB chunk (WBITS 24): at a distance of 2^24 - 16 the second copy is
    a match, one byte further it has to be stored again -- a longer distance would be read as a dictionary reference"""
    sizes = []
    for dist in (W.CAP_TAKEN, W.CAP_REFUSED):
        data = W.cap_input(dist)
        st = W.emu_stream(data, W.CAP_CHUNK, 9, grid=1)
        assert W.wbits_of(st) == 24
        W.decode_all(st, data)
        sizes.append(len(st))
    print("distance cap: %d bytes at 2^24 - 16, %d at 2^24 - 15" % tuple(sizes))
    assert sizes[0] <= W.CAP_NOISE + 8 * W.K                       # the match is taken: the noise is stored once
    assert sizes[1] - sizes[0] >= 64 * W.K


# ---- 5. worth having -----------------------------------------------------------------------------------------------------
def test_window_is_worth_having_on_text():
    win9, tab9 = text_size(9)[0], text_size(9, "level")[0]
    print("text 1 MiB, quality 9: window %d, table encoder %d" % (win9, tab9))
    assert win9 * 1.04 < tab9                                      # the bar between tiers of test_encoder_ratio_is_monotone_in_quality


def test_ratio_is_monotone_in_the_quality():
    sizes = [text_size(q)[0] for q in W.QUALITIES]
    print("text 1 MiB, qualities 9 / 10 / 11:", sizes)
    assert sizes[2] <= sizes[1] <= sizes[0]
    depth = W._lib().gpumt_brotli_win_depth
    assert [depth(q) for q in range(12)] == [0] * 9 + [16, 32, 64]


# ---- 6. determinism ------------------------------------------------------------------------------------------------------
def test_bytes_do_not_depend_on_the_grid():
    data, chunk = cases.text(500 * W.K, 31), 200000
    got = [W.emu_stream(data, chunk, 10, grid=g) for g in (1, 3, 8)]
    assert got[0] == got[1] == got[2]


def test_a_record_is_the_same_alone_and_inside_a_batch():
    """five chunks over three waves: the first wave builds the chains of chunks 0 and 3 with one head table"""
    chunk = 150000
    parts = [cases.text(chunk, 41), cases.text(chunk, 42), cases.rnd(chunk // 2, 43) * 2, cases.text(chunk, 41), cases.text(chunk - 7, 44)]
    recs, _ = W.emu_records(b"".join(parts), chunk, 9, grid=3)
    assert len(recs) == 5
    for k, part in enumerate(parts):
        alone, _ = W.emu_records(part, chunk, 9, grid=1)
        assert alone == [recs[k]], k
    assert recs[0] == recs[3]


# ---- 7. fallbacks and overrides ------------------------------------------------------------------------------------------
def test_qualities_below_9_are_the_table_encoder():
    data = cases.text(300 * W.K, 51)
    for q in (0, 4, 8):
        new, ran = W.emu_records(data, 200000, q)
        assert ran == 0 and new == W.emu_records(data, 200000, q, call="level")[0]


def test_refused_scratch_falls_back_to_the_table_encoder():
    data = cases.text(300 * W.K, 52)
    want = W.emu_records(data, 1 << 20, 11, call="level")[0]
    new, ran = W.emu_records(data, 1 << 20, 11, cap=4 * len(data) + 255)  # one byte short of GPUMT_BROTLI_WIN_SCRATCH(n)
    assert ran == 0 and new == want
    new, ran = W.emu_records(data, 1 << 20, 11, cap=4 * len(data) + 256)
    assert ran == 64 and new != want and len(new[0]) < len(want[0])


def test_depth_override():
    data = cases.text(200 * W.K, 53)
    assert W.emu_records(data, 1 << 20, 9, depth=64) == (W.emu_records(data, 1 << 20, 11)[0], 64)
    assert len(W.emu_stream(data, 1 << 20, 9, depth=1)) > len(W.emu_stream(data, 1 << 20, 9))


def test_depths_out_of_range_are_rejected():
    """the emulated boundary reads GPUMT_BROTLI_WIN_DEPTH where the device has gpumt_set_variant("brotli_win_depth")"""
    code = ("import sys; sys.path[:0] = %r\n"
            "import ctypes as C, numpy as np, emu_driver as E, helpers as H\n"
            "H.locked_make(%r, 'libzstdmt_emu_host.so')\n"
            "L = C.CDLL(%r)\n"
            "L.gpumt_zstd_slot_stride.restype = C.c_size_t; L.gpumt_zstd_slot_stride.argtypes = [C.c_size_t]\n"
            "h = C.c_void_p(); assert L.gpumt_open(0, C.byref(h)) == 0\n"
            "st = L.gpumt_zstd_slot_stride(1 << 20)\n"
            "inp = np.zeros(1000 + 64, np.uint8); slots = np.zeros(st, np.uint8); rl = np.zeros(1, np.uint32)\n"
            "print(L.gpumt_brotli_compress_batch_win(h, E._p(inp), C.c_size_t(1000), C.c_size_t(1 << 20), E._p(slots),\n"
            "      C.c_size_t(st), E._p(rl), 9, 0))\n") % (sys.path[:4], os.path.join(H.ROOT, "tests", "emu"),
                                                       os.path.join(H.ROOT, "tests", "emu", "libzstdmt_emu_host.so"))
    for text, want in (("257", "-3"), ("-1", "-3"), ("256", "0"), ("0", "0")):  # GPUMT_E_ARG where set_variant says -1
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=H.ROOT, timeout=600,
                           env=dict(os.environ, GPUMT_BROTLI_WIN_DEPTH=text))
        assert p.returncode == 0 and p.stdout.split()[-1] == want, (text, p.stdout, p.stderr[-800:])


# ---- 8. the strict and the shuffled emulator -----------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_win_under_the_strict_and_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "far_repeat_is_found or inside_a_batch or refused or (decompress_identical and (Q9 or Q11) and "
           "(bytes_ or empty or window_equals or chunk_200000 or chunk_1024 or zeros or period_300 or mixed))"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=3000, cwd=H.ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and "skipped" not in p.stdout, (p.stdout + p.stderr)[-1500:]
