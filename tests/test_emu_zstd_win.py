"""gpumt_zstd_compress_batch_win under the emulator: the chain plane against a model in plain Python, every stream
through three decoders, the far repeat the 128 KiB window cannot reach, the ratio bars between the table encoder and the
level groups, determinism in the grid and in the batch position, levels 1-9 and the scratch-refusal fallback -- and a
subset of it under the strict and the shuffled emulator."""
import os
import subprocess
import sys

import pytest

import helpers as H
import zstd_win as W
from golden import cases

SHAPES = W.shapes()
SOUPS = W.soups()
TEXT = cases.text(1 << 20, 5)
SIZES = {}


def text_size(level, call="win"):
    """the 1 MiB text at chunk 1 MiB, once per level and call (decoded where it is encoded)"""
    if (level, call) not in SIZES:
        st = W.emu_stream(TEXT, 1 << 20, level, grid=8, call=call)
        W.decode_all(st, TEXT, emu=level in (10, 19))
        SIZES[(level, call)] = (len(st), st)
    return SIZES[(level, call)]


# ---- the chain plane -----------------------------------------------------------------------------------------------------
PLANES = {
    "text": (cases.text(5000, 3) + bytes(300) + b"abc" * 200, 1 << 20),
    "twins_in_a_step": (bytes(200) + b"ab" * 100 + cases.rep(cases.rnd(7, 2), 400) + b"xyz", 1 << 20),
    "three_chunks_one_wave": (cases.text(2500, 4) * 3, 2500),        # the same bytes: an old head would be followed
    "ragged_last_chunk": (cases.text(2000, 5) + bytes(100) + cases.text(777, 5), 1000),
    "shorter_than_a_hash": (b"abcab", 1 << 20),
    "chunks_of_5": (b"aaaaaaaaaaaaaaaaaaaaaa", 5),
}


@pytest.mark.parametrize("name", sorted(PLANES))
def test_chain_plane_is_the_models(name):
    """prev[p] is the nearest earlier position of the same chunk with the same hash; lanes of one step chain to each
    other in position order; a chunk's last five positions and its first occurrence of a hash have none; no entry of
    one chunk points into another (the head table is reset per chunk); the grid does not matter"""
    data, chunk = PLANES[name]
    want = W.model_plane(data, chunk)
    for grid in (1, 3):
        got = W.emu_plane(data, chunk, grid)
        assert (got == want).all(), (name, grid, [(p, int(got[p]), int(want[p])) for p in range(len(data)) if got[p] != want[p]][:5])
    if name == "twins_in_a_step":
        assert [int(x) for x in want[1:64]] == list(range(63))       # zeros: every lane chains to the lane below it


# ---- decompress-identical ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", W.LEVELS, ids=lambda lv: "L%d" % lv)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_decompress_identical(name, level):
    data, chunk = SHAPES[name]
    st = W.emu_stream(data, chunk, level)
    W.decode_all(st, data)
    if name in ("zeros_300k", "period_300"):
        assert len(st) < len(data) // 100


@pytest.mark.parametrize("name", sorted(SOUPS))
def test_soup(name):
    data, chunk, rng = SOUPS[name]
    st = W.emu_stream(data, chunk, rng.choice(W.LEVELS), grid=rng.choice((1, 3, 8)))
    W.decode_all(st, data)


def test_a_match_never_takes_its_source_from_the_neighbour_chunk():
    """every record decodes on its own: chunk k's frame alone gives chunk k"""
    data, chunk = SHAPES["chunk_1024"]
    recs, ran = W.emu_records(data, chunk, 19, grid=8)
    assert ran == 64 and len(recs) == 300
    for k in (0, 1, 2, 150, 299):
        assert H.oracle_zstdmt_decompress(recs[k], chunk + 64) == data[k * chunk:(k + 1) * chunk]


# ---- far repeat ----------------------------------------------------------------------------------------------------------
def test_far_repeat_is_found():
    """192 KiB of noise twice in one 1 MiB chunk: the second copy is one long match 192 KiB back (a sequence covers up to
    131 074 bytes; libzstd writes 196 649 bytes), where the table encoder, whose matches stay in their 128 KiB block,
    stores both copies: 393 246 bytes"""
    st = W.emu_stream(W.FAR, 1 << 20, 10)
    print("far repeat: %d bytes, table encoder %d" % (len(st), len(W.emu_stream(W.FAR, 1 << 20, 10, call="level"))))
    W.decode_all(st, W.FAR)
    assert len(st) <= W.FAR_BOUND


# ---- worth having --------------------------------------------------------------------------------------------------------
def test_window_is_worth_having_on_text():
    win10, tab10 = text_size(10)[0], text_size(10, "level")[0]
    print("text 1 MiB, level 10: window %d, table encoder %d" % (win10, tab10))
    assert win10 * 1.04 < tab10                                   # the bar between tiers of test_emu_ratio_is_monotone_in_level


def test_ratio_is_monotone_in_the_level_groups():
    sizes = [text_size(lv)[0] for lv in (10, 13, 16, 19)]
    print("text 1 MiB, levels 10 / 13 / 16 / 19:", sizes)
    assert sizes[3] <= sizes[2] <= sizes[1] <= sizes[0]


def test_levels_of_one_group_give_the_same_bytes():
    assert text_size(22)[1] == text_size(19)[1]
    data = cases.text(200 * W.K, 21)
    for a, b in ((10, 12), (13, 15), (16, 18)):
        assert W.emu_stream(data, 1 << 20, a) == W.emu_stream(data, 1 << 20, b)
    depth = W._lib().gpumt_zstd_win_depth
    assert [depth(lv) for lv in (1, 9, 10, 12, 13, 15, 16, 18, 19, 22)] == [0, 0, 8, 8, 16, 16, 32, 32, 64, 64]


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_bytes_do_not_depend_on_the_grid():
    data, chunk = cases.text(500 * W.K, 31), 200000
    got = [W.emu_stream(data, chunk, 13, grid=g) for g in (1, 3, 8)]
    assert got[0] == got[1] == got[2]


def test_a_record_is_the_same_alone_and_inside_a_batch():
    """five chunks over three waves: the first wave builds the chains of chunks 0 and 3 with one head table"""
    chunk = 150000
    parts = [cases.text(chunk, 41), cases.text(chunk, 42), cases.rnd(chunk // 2, 43) * 2, cases.text(chunk, 41), cases.text(chunk - 7, 44)]
    recs, _ = W.emu_records(b"".join(parts), chunk, 10, grid=3)
    assert len(recs) == 5
    for k, part in enumerate(parts):
        alone, _ = W.emu_records(part, chunk, 10, grid=1)
        assert alone == [recs[k]], k
    assert recs[0] == recs[3]


# ---- levels 1-9 and the fallback -----------------------------------------------------------------------------------------
def test_levels_below_10_are_the_table_encoder():
    data = cases.text(300 * W.K, 51)
    for lv in (1, 3, 9):
        new, ran = W.emu_records(data, 200000, lv)
        assert ran == 0 and new == W.emu_records(data, 200000, lv, call="level")[0]


def test_refused_scratch_falls_back_to_the_table_encoder():
    data = cases.text(300 * W.K, 52)
    want = W.emu_records(data, 1 << 20, 19, call="level")[0]
    new, ran = W.emu_records(data, 1 << 20, 19, cap=4 * len(data))        # one byte short of the plane
    assert ran == 0 and new == want
    new, ran = W.emu_records(data, 1 << 20, 19, cap=4 * len(data) + 256)
    assert ran == 64 and new != want and len(new[0]) < len(want[0])


def test_depth_override():
    data = cases.text(200 * W.K, 53)
    assert W.emu_records(data, 1 << 20, 10, depth=64) == (W.emu_records(data, 1 << 20, 19)[0], 64)
    assert len(W.emu_stream(data, 1 << 20, 10, depth=1)) > len(W.emu_stream(data, 1 << 20, 10))


# ---- the strict and the shuffled emulator --------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_win_under_the_strict_and_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "chain_plane or far_repeat or inside_a_batch or refused or (decompress_identical and (L10 or L19) and "
           "(bytes_ or empty or window_equals or chunk_200000 or chunk_1024 or zeros or period_300 or mixed))"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=3000, cwd=H.ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and "skipped" not in p.stdout, (p.stdout + p.stderr)[-1500:]
