"""The segment-parallel chain build under the emulator: the three launches of enc_win_chain_par.h write the plane of the
serial kernel and of the Python model word for word -- at three segment sizes and two grids, from head tables that start as
garbage -- and both window encoders write the same records with GPUMT_WIN_CHAIN_PAR set, unset, and with the head tables
refused; a subset once more under the strict and the shuffled emulator."""
import os
import subprocess
import sys

import pytest

import helpers as H
import win_chain as W

SHAPES = W.shared_shapes()
MODEL = {}
CODECS = {"zstd_L10": ("zstd", 10), "zstd_L19": ("zstd", 19), "brotli_Q9": ("brotli", 9), "brotli_Q11": ("brotli", 11)}


def model(name):
    if name not in MODEL:
        data, chunk = SHAPES[name]
        MODEL[name] = W.model_plane(data, chunk)
        assert (W.emu_plane(data, chunk) == MODEL[name]).all()     # the serial kernel, once per shape
    return MODEL[name]


@pytest.mark.parametrize("seg_log", (12, 13, 16))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plane_is_the_serial_kernels_and_the_models(name, seg_log):
    data, chunk = SHAPES[name]
    want = model(name)
    for grid in (1, 3):
        got = W.emu_plane_par(data, chunk, seg_log, grid)
        assert (got == want).all(), (name, seg_log, grid,
                                     [(p, int(got[p]), int(want[p])) for p in range(len(data)) if got[p] != want[p]][:5])


def test_the_shapes_reach_the_stitching():
    """what the shape list claims, from the model: links across a segment border, across many, and positions that stay NONE"""
    S = 1 << W.SEG_LOG
    zeros = model("zeros_300k")
    assert all(int(zeros[k * S]) == k * S - 1 for k in range(1, 70))
    far = model("period_65537")
    # 65537 positions per period over 2^15 hashes: about e^-2 of them meet no other position of their period first
    back = [p for p in range(65537, 300 * W.K - 5) if int(far[p]) == p - 65537]
    assert len(back) > 10000 and all((p >> W.SEG_LOG) - ((p - 65537) >> W.SEG_LOG) in (16, 17) for p in back)
    rnd = model("rnd_40k")
    assert sum(1 for p in range(S, 40 * W.K - 5) if int(rnd[p]) == W.ZW.NONE) > 1000       # about 4096 / e first occurrences
    for n in (4097, 4096 + 5, 4096 + 6):
        pl = model("one_chunk_%d" % n)
        assert (pl[n - 5:] == W.ZW.NONE).all()
    assert W.par_scratch(2 * 65536 + 5000, 65536, 12) == 3 * 16 * (4 << 13)       # 16 segments per chunk, stride by the chunk
    assert W.par_scratch(4096, 1 << 20, 12) == 0 and W.par_scratch(4097, 1 << 20, 12) == 2 * (4 << 12)
    assert W.par_scratch(0, 1 << 20, 12) == 0 and W.par_scratch(300 * W.K, 1024, 12) == 0


@pytest.mark.parametrize("codec", sorted(CODECS))
@pytest.mark.parametrize("name", sorted(W.shapes()))
def test_records_are_the_same_with_the_variable_set(name, codec, capfd):
    data, chunk = SHAPES[name]
    kind, level = CODECS[codec]
    off = W.emu_gpumt_records(kind, data, chunk, level)
    assert W.chain_lines(capfd.readouterr().err) == []
    on = W.emu_gpumt_records(kind, data, chunk, level, par=12)
    lines = W.chain_lines(capfd.readouterr().err)
    assert on == off
    heads = W.par_scratch(len(data), chunk, 12)
    assert len(lines) == 1 and lines[0]["seg_log"] == 12 and lines[0]["heads"] == heads and lines[0]["serial"] == (heads == 0)
    if heads:
        assert lines[0]["segments"] > len(on)


@pytest.mark.parametrize("codec", sorted(CODECS))
def test_refused_head_tables_leave_the_serial_kernel(codec, capfd):
    kind, level = CODECS[codec]
    for name in ("one_chunk_4101", "short_last_chunk"):
        data, chunk = SHAPES[name]
        off = W.emu_gpumt_records(kind, data, chunk, level)
        capfd.readouterr()
        capped = W.emu_gpumt_records(kind, data, chunk, level, par=12, cap=1)
        lines = W.chain_lines(capfd.readouterr().err)
        assert capped == off and len(lines) == 1 and lines[0]["serial"] == 1 and lines[0]["heads"] > 1


def test_other_values_of_the_variable_are_off(capfd):
    data, chunk = SHAPES["one_chunk_8192"]
    off = W.emu_gpumt_records("zstd", data, chunk, 10)
    capfd.readouterr()
    for text in ("", "0", "yes", "12x", "11", "25", "-1"):
        assert W.emu_gpumt_records("zstd", data, chunk, 10, par=text) == off
        assert W.chain_lines(capfd.readouterr().err) == [], text
    for text, seg_log in (("1", 20), ("24", 24), ("16", 16)):
        assert W.emu_gpumt_records("zstd", data, chunk, 10, par=text) == off
        lines = W.chain_lines(capfd.readouterr().err)
        assert len(lines) == 1 and lines[0]["seg_log"] == seg_log, text


@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_under_the_strict_and_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "(plane_is and (one_chunk or short_last or bytes_ or empty or rnd_40k)) or (records_are and one_chunk_4097) or "
           "(refused and L10)"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=3000, cwd=H.ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and "skipped" not in p.stdout, (p.stdout + p.stderr)[-1500:]
