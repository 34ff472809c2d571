"""Helpers of the whole-chunk-window tests through BROTLIMT_compressCCtx (TEST CODE ONLY): one text compressed in a process
of its own with GPUMT_BROTLI_WIN holding what the test says (None = unset), over the emulated boundary or the device."""
import base64
import ctypes as C
import json
import os
import subprocess
import sys

import helpers as H
from golden import cases

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
CHUNK = 200000


def api_text():
    return cases.text(450 * 1024, 61)                     # three records, the last one short


def _run(kind, levels):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    L = H.bind_lz4mt(C.CDLL(path), "BROTLIMT_")
    res = {}
    for lv in levels:
        sys.stderr.write("CASE %d\n" % lv)
        sys.stderr.flush()
        rv, out, io, stats = H.brotlimt_compress_via(L, api_text(), CHUNK, threads=2, level=lv)
        res[str(lv)] = dict(rv=rv, stream=base64.b64encode(out).decode(), stats=list(stats),
                            reads=[list(r) for r in io.reads], writes=list(io.writes))
    print(json.dumps(res))


def run_api(kind, win, levels):
    """-> {level: dict(rv, stream, stats, reads, writes, trace = the [gpumt brotli win] lines of that call)}"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_TRACE="1")
    for k in ("GPUMT_BROTLI_WIN", "GPUMT_BROTLI_WIN_DEPTH", "GPUMT_BROTLI_WIN_CAP", "GPUMT_BATCH_MB", "GPUMT_BATCH_KB"):
        env.pop(k, None)
    if win is not None:
        env["GPUMT_BROTLI_WIN"] = win
    code = "import sys; sys.path[:0] = %r; import brotli_win_api as A; A._run(%r, %r)" % (sys.path[:4], kind, list(levels))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = {int(k): v for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()}
    lv = None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            lv = int(line[5:])
            res[lv]["trace"] = []
        elif line.startswith("[gpumt brotli win]") and lv is not None:
            w = line.split()
            res[lv]["trace"].append(dict(records=int(w[4]), depth=int(w[6]), plane=int(w[8]), fallback=int(w[10])))
    for v in res.values():
        v["stream"] = base64.b64decode(v["stream"])
    return res


def check_legs(kind, decode):
    """the legs of the issue: quality 11 with the variable is smaller, decodes and keeps the callback trace; unset, 0, 2
    and yes are the parent's path byte for byte; quality 5 does not change.  decode(stream) -> content"""
    data = api_text()
    off = run_api(kind, None, (11, 5))
    on = run_api(kind, "1", (11, 5))
    a, b = on[11], off[11]
    assert a["rv"] == 0 and b["rv"] == 0
    print("quality 11 through the API: %d bytes with GPUMT_BROTLI_WIN=1, %d without" % (len(a["stream"]), len(b["stream"])))
    assert len(a["stream"]) * 1.04 < len(b["stream"])
    assert decode(a["stream"]) == data and decode(b["stream"]) == data
    assert H.oracle_brotlimt_decompress(a["stream"], len(data) + 65536) == data
    if H.have_bref():
        rv, out, _, _ = H.brotlimt_decompress_via(H.bref(), a["stream"], threads=2)
        assert rv == 0 and out == data
    assert a["reads"] == b["reads"] and len(a["writes"]) == len(b["writes"]) == 3
    assert a["stats"][:2] == b["stats"][:2] == [3, len(data)] and a["stats"][2] == len(a["stream"])
    assert a["trace"] and all(t["depth"] == 64 and t["fallback"] == 0 and t["plane"] > 0 for t in a["trace"])
    assert sum(t["records"] for t in a["trace"]) == 3 and b["trace"] == []
    assert on[5]["stream"] == off[5]["stream"] and on[5]["trace"] == []
    for text in ("0", "2", "yes"):
        other = run_api(kind, text, (11,))
        assert other[11]["stream"] == b["stream"] and other[11]["trace"] == [], text
