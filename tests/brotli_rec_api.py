"""Helpers of the span-index tests through BROTLIMT_compressCCtx / BROTLIMT_decompressDCtx (TEST CODE ONLY): one input
compressed and decompressed in a process of its own with GPUMT_BROTLI_INDEX / GPUMT_BROTLI_REC_PAR holding what the test
says (None = unset), over the emulated boundary or the device."""
import base64
import ctypes as C
import json
import os
import subprocess
import sys

import brotli_rec as R
import helpers as H

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
CHUNK = 1 << 20
LEVEL = 5


def api_data():
    return R.light((1 << 20) + 3 * R.BLOCK + 77, 90)      # two records: eight spans and four


def _run(kind, stream_b64):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    L = H.bind_lz4mt(C.CDLL(path), "BROTLIMT_")
    sys.stderr.write("CASE compress\n")
    sys.stderr.flush()
    rv, out, io, stats = H.brotlimt_compress_via(L, api_data(), CHUNK, threads=2, level=LEVEL)
    src = base64.b64decode(stream_b64) if stream_b64 else out
    sys.stderr.write("CASE decompress\n")
    sys.stderr.flush()
    drv, dout, dio, dstats = H.brotlimt_decompress_via(L, src, threads=2)
    print(json.dumps(dict(rv=rv, stream=base64.b64encode(out).decode(), stats=list(stats), reads=[list(r) for r in io.reads],
                          writes=list(io.writes), drv=drv, dout=base64.b64encode(dout).decode(), dstats=list(dstats),
                          dreads=[list(r) for r in dio.reads], dwrites=list(dio.writes))))


def run_api(kind, index=None, rec_par=None, min_spans=None, stream=None):
    """compress api_data(), then decompress `stream` (default: what was just written) -> dict with both callback traces and
    `trace`, the [gpumt brotli rec] lines of the decompression"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_TRACE="1")
    for k in ("GPUMT_BROTLI_WIN", "GPUMT_BROTLI_INDEX", "GPUMT_BROTLI_REC_PAR", "GPUMT_BROTLI_REC_MIN_SPANS", "GPUMT_BROTLI_REC_CAP",
              "GPUMT_BATCH_MB", "GPUMT_BATCH_KB"):
        env.pop(k, None)
    for k, v in (("GPUMT_BROTLI_INDEX", index), ("GPUMT_BROTLI_REC_PAR", rec_par), ("GPUMT_BROTLI_REC_MIN_SPANS", min_spans)):
        if v is not None:
            env[k] = v
    code = "import sys; sys.path[:0] = %r; import brotli_rec_api as A; A._run(%r, %r)" % (
        sys.path[:4], kind, base64.b64encode(stream).decode() if stream else "")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    res["trace"] = R.trace_stats(p.stderr[p.stderr.index("CASE decompress"):].splitlines())
    res["stream"], res["dout"] = base64.b64decode(res["stream"]), base64.b64decode(res["dout"])
    return res


def check_legs(kind):
    data = api_data()
    off = run_api(kind)
    on = run_api(kind, index="1", rec_par="1")
    assert off["rv"] == on["rv"] == 0 and off["drv"] == on["drv"] == 0 and off["dout"] == on["dout"] == data
    # the index: 8 bytes per block and the 10 / 10 of header and trailer in the two records; nothing else changes
    assert len(on["stream"]) - len(off["stream"]) == R.index_bytes(8) + R.index_bytes(4) <= 8 * 12 + 2 * 13
    recs = [R.split_index(R.payload_of(r)[0]) for r in R.records_of(on["stream"])]
    assert [len(e) for _, e in recs] == [8, 4]
    assert [p for p, _ in recs] == [R.payload_of(r)[0] for r in R.records_of(off["stream"])]
    assert on["reads"] == off["reads"] and len(on["writes"]) == len(off["writes"]) == 2
    assert on["stats"][:2] == off["stats"][:2] and on["stats"][2] == len(on["stream"])
    assert off["trace"] == [] and sum(t["kept"] for t in on["trace"]) == 2 and sum(t["spans"] for t in on["trace"]) == 12
    # everyone else reads the indexed stream
    assert H.oracle_brotlimt_decompress(on["stream"], len(data) + 65536) == data
    if H.have_bref():
        rv, out, _, _ = H.brotlimt_decompress_via(H.bref(), on["stream"], threads=2)
        assert rv == 0 and out == data
    # the same stream with and without the par decoder: the same callback trace, statistics and bytes
    ser = run_api(kind, stream=on["stream"])
    par = run_api(kind, rec_par="1", stream=on["stream"])
    low = run_api(kind, rec_par="1", min_spans="5", stream=on["stream"])
    for r in (par, low):
        assert r["drv"] == ser["drv"] == 0 and r["dout"] == ser["dout"] == data
        assert r["dwrites"] == ser["dwrites"] and r["dreads"] == ser["dreads"] and r["dstats"] == ser["dstats"]
    assert ser["trace"] == [] and sum(t["kept"] for t in par["trace"]) == 2 and sum(t["kept"] for t in low["trace"]) == 1
    # a stream without index through the par decoder, and other texts in the variables: the parent's path
    plain = run_api(kind, rec_par="1")
    assert plain["stream"] == off["stream"] and plain["dout"] == data and sum(t["par"] for t in plain["trace"]) == 0
    for text in ("0", "2", "yes"):
        other = run_api(kind, index=text, rec_par=text)
        assert other["stream"] == off["stream"] and other["trace"] == [] and other["dout"] == data, text
