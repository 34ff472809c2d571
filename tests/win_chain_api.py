"""Helpers of the segment-parallel chain build tests through ZSTDCB_compressCCtx and BROTLIMT_compressCCtx (TEST CODE ONLY):
one text compressed in a process of its own with GPUMT_{ZSTD,BROTLI}_WIN=1 and GPUMT_WIN_CHAIN_PAR holding what the test says
(None = unset), over the emulated boundary or the device."""
import base64
import ctypes as C
import json
import os
import subprocess
import sys

import helpers as H
from golden import cases

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
CHUNK = 100003                                            # 25 segments of 4 KiB, the last one 1699 positions
CODECS = {"zstd": ("ZSTDCB_", 19, "GPUMT_ZSTD_WIN"), "brotli": ("BROTLIMT_", 11, "GPUMT_BROTLI_WIN")}


def api_text():
    return cases.text(220 * 1024, 63)                     # three records, the last one short


def _run(kind, codec):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    prefix, level, _ = CODECS[codec]
    L = H.bind_lz4mt(C.CDLL(path), prefix)
    via = H.zstdmt_compress_via if codec == "zstd" else H.brotlimt_compress_via
    rv, out, io, stats = via(L, api_text(), CHUNK, threads=2, level=level)
    print(json.dumps(dict(rv=rv, stream=base64.b64encode(out).decode(), stats=list(stats))))


def run_api(kind, codec, par):
    """-> dict(rv, stream, stats, win = the [gpumt <codec> win] lines, chain = the [gpumt win chain] lines as dicts)"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_TRACE="1")
    for k in ("GPUMT_ZSTD_WIN", "GPUMT_ZSTD_WIN_DEPTH", "GPUMT_ZSTD_WIN_CAP", "GPUMT_BROTLI_WIN", "GPUMT_BROTLI_WIN_DEPTH",
              "GPUMT_BROTLI_WIN_CAP", "GPUMT_WIN_CHAIN_PAR", "GPUMT_WIN_CHAIN_CAP", "GPUMT_BATCH_MB", "GPUMT_BATCH_KB"):
        env.pop(k, None)
    env[CODECS[codec][2]] = "1"
    if par is not None:
        env["GPUMT_WIN_CHAIN_PAR"] = par
    code = "import sys; sys.path[:0] = %r; import win_chain_api as A; A._run(%r, %r)" % (sys.path[:4], kind, codec)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    res["stream"] = base64.b64decode(res["stream"])
    res["win"], res["chain"] = [], []
    for line in p.stderr.splitlines():
        w = line.split()
        if line.startswith("[gpumt %s win]" % codec):
            res["win"].append(line)
        elif line.startswith("[gpumt win chain]"):
            res["chain"].append(dict(segments=int(w[4]), seg_log=int(w[6]), heads=int(w[8]), serial=int(w[10])))
    return res


def check_legs(kind, codec, decode):
    """the stream is the same with GPUMT_WIN_CHAIN_PAR=12 and without; the chain line is there with serial 0 and more
    segments than records in the first case and absent in the second; other text is unset.  decode(stream) -> content"""
    data = api_text()
    off = run_api(kind, codec, None)
    on = run_api(kind, codec, "12")
    assert on["rv"] == 0 and off["rv"] == 0 and on["stream"] == off["stream"] and on["stats"] == off["stats"]
    assert decode(on["stream"]) == data
    assert off["chain"] == [] and off["win"] and on["win"] == off["win"]        # the existing line, character for character
    assert on["chain"] and len(on["chain"]) == len(on["win"])
    records = sum(int(line.split()[4]) for line in on["win"])
    assert records == 3 and sum(c["segments"] for c in on["chain"]) > records
    assert all(c["serial"] == 0 and c["seg_log"] == 12 and c["heads"] > 0 for c in on["chain"])
    other = run_api(kind, codec, "yes")
    assert other["stream"] == off["stream"] and other["chain"] == [] and other["win"] == off["win"]
