"""Helpers of the block-parallel record path tests through ZSTDCB_decompressDCtx (TEST CODE ONLY): one zstd-mt stream
decoded in a process of its own with GPUMT_ZSTD_REC_PAR holding what the test says (None = unset), over the emulated
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
import zstd_blocks as Z
from golden import cases

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
CHUNK = 400000
VARS = ("GPUMT_ZSTD_REC_PAR", "GPUMT_ZSTD_REC_MIN_BLOCKS", "GPUMT_ZSTD_REC_SLICE_BLOCKS", "GPUMT_BATCH_MB", "GPUMT_BATCH_KB")


def api_text():
    return cases.text(900 * 1024, 67)                     # three records: 400 000, 400 000 and 121 600 bytes


def _lib(kind):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    return H.bind_lz4mt(C.CDLL(path), "ZSTDCB_")


def _compress(kind, path):
    rv, out, _, _ = H.zstdmt_compress_via(_lib(kind), api_text(), CHUNK, threads=2, level=1)
    assert rv == 0
    with open(path, "wb") as f:
        f.write(out)


def _decode(kind, path, threads):
    with open(path, "rb") as f:
        stream = f.read()
    rv, out, io, stats = H.zstdmt_decompress_via(_lib(kind), stream, threads=threads)
    print(json.dumps(dict(rv=rv, out=base64.b64encode(out).decode(), stats=list(stats), reads=[list(r) for r in io.reads],
                          writes=list(io.writes))))


def _child(code, env):
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import zstd_rec_api as A; %s" % (sys.path[:4], code)],
                       capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    return p


def _env(rec_par=None, batch_kb=None, min_blocks=None):
    env = dict(os.environ, GPUMT_TRACE="1")
    for k in VARS:
        env.pop(k, None)
    if rec_par is not None:
        env["GPUMT_ZSTD_REC_PAR"] = rec_par
    if batch_kb is not None:
        env["GPUMT_BATCH_KB"] = str(batch_kb)
    if min_blocks is not None:
        env["GPUMT_ZSTD_REC_MIN_BLOCKS"] = str(min_blocks)
    return env


def compress(kind, path):
    """the text through ZSTDCB_compressCCtx at chunk 400 000 -> the stream, also left in `path`"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    _child("A._compress(%r, %r)" % (kind, path), _env())
    with open(path, "rb") as f:
        return f.read()


def decode(kind, path, rec_par, threads=2, batch_kb=None, min_blocks=None):
    """-> dict(rv, out, stats, reads, writes, trace = the [gpumt zstd rec] lines of the call as dicts)"""
    p = _child("A._decode(%r, %r, %r)" % (kind, path, threads), _env(rec_par, batch_kb, min_blocks))
    r = json.loads(p.stdout.strip().splitlines()[-1])
    r["out"] = base64.b64decode(r["out"])
    r["trace"] = []
    for line in p.stderr.splitlines():
        if line.startswith("[gpumt zstd rec]"):
            w = line.split()
            r["trace"].append({w[i]: int(w[i + 1]) for i in range(3, 13, 2)})
    return r


def same(a, b):
    return all(a[k] == b[k] for k in ("rv", "out", "stats", "reads", "writes"))


def check_stream(kind, path, data, eligible):
    """the five texts of the variable give the same content, return value, counters and callback lists; the trace line
    appears only for "1", where `eligible` records took the block stages"""
    runs = {t: decode(kind, path, t) for t in (None, "1", "0", "2", "yes")}
    base = runs[None]
    assert base["rv"] == 0 and base["out"] == data
    for t, r in runs.items():
        assert same(r, base), t
        if t == "1":
            assert r["trace"] and sum(x["par"] for x in r["trace"]) == eligible, r["trace"]
            assert all(x["fallback"] == 0 for x in r["trace"])
        else:
            assert r["trace"] == [], t
    return base


def block_counts(stream):
    ro, rl = E.walk_records(stream)
    return [len(Z.walk(stream[int(o) + 12:int(o) + int(n)])["blocks"]) for o, n in zip(ro, rl)]


def check_legs(kind):
    """The device encoder writes a 128 KiB unit as several Compressed blocks, so its three records hold more blocks than
    the 4, 4 and 1 of libzstd's frames: at the default threshold of 4 all three are eligible, and with the threshold above
    the last record's count two are.  The reference build's stream of the same text is 4, 4 and 1: two eligible."""
    data = api_text()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "own.zstdmt")
        counts = block_counts(compress(kind, path))
        assert len(counts) == 3 and counts[2] >= 4 and min(counts[:2]) > counts[2], counts
        base = check_stream(kind, path, data, 3)
        assert base["stats"][0] == 3
        two = decode(kind, path, "1", min_blocks=counts[2] + 1)
        assert same(two, base) and sum(x["par"] for x in two["trace"]) == 2
        assert sum(x["blocks"] for x in two["trace"]) == sum(counts[:2])
        # one thread; and every record a batch of its own
        one = decode(kind, path, "1", threads=1)
        assert one["rv"] == 0 and one["out"] == data and one["stats"] == base["stats"]
        assert sum(x["par"] for x in one["trace"]) == 3
        each = decode(kind, path, "1", batch_kb=16)
        assert each["rv"] == 0 and each["out"] == data and each["stats"] == base["stats"]
        assert [x["records"] for x in each["trace"]] == [1, 1, 1] and sum(x["par"] for x in each["trace"]) == 3
        # libzstd-shaped frames whatever this machine holds: the same text as Raw blocks of 128 KiB, 4, 4 and 1 per record
        hpath = os.path.join(d, "raw.zstdmt")
        hand = b"".join(H.mt_record(Z.frame_of([("raw", data[i + j:min(i + j + 131072, i + CHUNK)])
                                                for j in range(0, min(CHUNK, len(data) - i), 131072)],
                                               csize=min(CHUNK, len(data) - i))) for i in range(0, len(data), CHUNK))
        assert block_counts(hand) == [4, 4, 1]
        with open(hpath, "wb") as f:
            f.write(hand)
        raw = decode(kind, hpath, "1")
        assert raw["rv"] == 0 and raw["out"] == data and sum(x["par"] for x in raw["trace"]) == 2
        assert same(decode(kind, hpath, None), raw)
        if H.have_zref():
            # the reference build's own stream of the same text: libzstd's frames, level 3
            rv, ref_stream, _, _ = H.zstdmt_compress_via(H.zref(), data, CHUNK, threads=2, level=3)
            assert rv == 0 and block_counts(ref_stream) == [4, 4, 1]
            rpath = os.path.join(d, "ref.zstdmt")
            with open(rpath, "wb") as f:
                f.write(ref_stream)
            check_stream(kind, rpath, data, 2)
