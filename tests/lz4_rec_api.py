"""Helpers of the block-parallel record path tests through LZ4MT_decompressDCtx (TEST CODE ONLY): one lz4-mt stream
decoded in a process of its own with GPUMT_LZ4_REC_PAR holding what the test says (None = unset), over the emulated
boundary or the device."""
import base64
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import emu_driver as E
import helpers as H
import lz4_rec as K
from golden import cases

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
CHUNK = 400000
VARS = ("GPUMT_LZ4_REC_PAR", "GPUMT_LZ4_REC_SEG", "GPUMT_LZ4_REC_MIN_BLOCKS", "GPUMT_LZ4_REC_SLICE_BLOCKS", "GPUMT_BATCH_MB",
        "GPUMT_BATCH_KB")
TAG = "[gpumt lz4 rec]"


def api_text():
    return cases.text(900 * 1024, 67)                     # three records: 400 000, 400 000 and 121 600 bytes


def _lib(kind):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    return H.bind_lz4mt(C.CDLL(path))


def _compress(kind, path):
    rv, out, _, _ = H.lz4mt_compress_via(_lib(kind), api_text(), CHUNK, threads=2, level=1)
    assert rv == 0
    with open(path, "wb") as f:
        f.write(out)


def _decode(kind, path, threads):
    with open(path, "rb") as f:
        stream = f.read()
    rv, out, io, stats = H.lz4mt_decompress_via(_lib(kind), stream, threads=threads)
    print(json.dumps(dict(rv=rv, out=base64.b64encode(out).decode(), stats=list(stats), reads=[list(r) for r in io.reads],
                          writes=list(io.writes))))


def _child(code, env):
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import lz4_rec_api as A; %s" % (sys.path[:4], code)],
                       capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    return p


def _env(rec_par=None, batch_kb=None, min_blocks=None, seg=None):
    env = dict(os.environ, GPUMT_TRACE="1")
    for k in VARS:
        env.pop(k, None)
    if rec_par is not None:
        env["GPUMT_LZ4_REC_PAR"] = rec_par
    if batch_kb is not None:
        env["GPUMT_BATCH_KB"] = str(batch_kb)
    if min_blocks is not None:
        env["GPUMT_LZ4_REC_MIN_BLOCKS"] = str(min_blocks)
    if seg is not None:
        env["GPUMT_LZ4_REC_SEG"] = str(seg)
    return env


def compress(kind, path):
    """the text through LZ4MT_compressCCtx at chunk 400 000 -> the stream, also left in `path`"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    _child("A._compress(%r, %r)" % (kind, path), _env())
    with open(path, "rb") as f:
        return f.read()


def decode(kind, path, rec_par, threads=2, batch_kb=None, min_blocks=None, seg=None):
    """-> dict(rv, out, stats, reads, writes, trace = the [gpumt lz4 rec] lines of the call as dicts)"""
    p = _child("A._decode(%r, %r, %r)" % (kind, path, threads), _env(rec_par, batch_kb, min_blocks, seg))
    r = json.loads(p.stdout.strip().splitlines()[-1])
    r["out"] = base64.b64decode(r["out"])
    r["trace"] = K.trace_stats(p.stderr.splitlines())
    return r


def same(a, b):
    return all(a[k] == b[k] for k in ("rv", "out", "stats", "reads", "writes"))


def check_stream(kind, path, data, eligible, blocks, min_blocks=4):
    """the five texts of the variable give the same content, return value, counters and callback lists; the trace line
    appears only for "1", where `eligible` records with `blocks` blocks took the block stages (threshold `min_blocks`)"""
    runs = {t: decode(kind, path, t, min_blocks=min_blocks) for t in (None, "1", "0", "2", "")}
    base = runs[None]
    assert base["rv"] == 0 and base["out"] == data
    for t, r in runs.items():
        assert same(r, base), t
        if t == "1":
            assert r["trace"] and sum(x["par"] for x in r["trace"]) == eligible, r["trace"]
            assert sum(x["blocks"] for x in r["trace"]) == blocks
            assert all(x["fallback"] == 0 and x["route"] == "par" for x in r["trace"])
        else:
            assert r["trace"] == [], t
    return base


def block_counts(stream):
    ro, rl = E.walk_records(stream)
    return [K.nblocks(stream[int(o) + 12:int(o) + int(n)]) for o, n in zip(ro, rl)]


def check_legs(kind):
    """The text at chunk 400 000 is three records of 7, 7 and 2 blocks of 64 KiB: with the threshold at 4 two are eligible,
    with the threshold at 2 all three are, and at the default the records that have as many blocks."""
    data = api_text()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "own.lz4mt")
        counts = block_counts(compress(kind, path))
        assert counts == [7, 7, 2]
        base = check_stream(kind, path, data, 2, 14)
        assert base["stats"][0] == 3
        dflt = decode(kind, path, "1")
        assert same(dflt, base) and dflt["trace"] and all(x["fallback"] == 0 for x in dflt["trace"])
        assert sum(x["blocks"] for x in dflt["trace"]) == sum(c for c in counts if c >= K.DEFAULT_MIN_BLOCKS)
        three = decode(kind, path, "1", min_blocks=2)
        assert same(three, base) and sum(x["par"] for x in three["trace"]) == 3
        assert sum(x["blocks"] for x in three["trace"]) == 16
        # the seg route, and every record a batch of its own
        seg = decode(kind, path, "1", seg=1, min_blocks=4)
        assert same(seg, base) and sum(x["par"] for x in seg["trace"]) == 2 and all(x["route"] == "seg" for x in seg["trace"])
        each = decode(kind, path, "1", batch_kb=16, min_blocks=2)
        assert each["rv"] == 0 and each["out"] == data and each["stats"] == base["stats"]
        assert [x["records"] for x in each["trace"]] == [1, 1, 1] and [x["par"] for x in each["trace"]] == [1, 1, 1]
        if H.have_ref():
            # the reference build's own stream of the same text
            rv, ref_stream, _, _ = H.lz4mt_compress_via(H.ref(), data, CHUNK, threads=2, level=1)
            assert rv == 0 and block_counts(ref_stream) == [7, 7, 2]
            rpath = os.path.join(d, "ref.lz4mt")
            with open(rpath, "wb") as f:
                f.write(ref_stream)
            check_stream(kind, rpath, data, 2, 14)
