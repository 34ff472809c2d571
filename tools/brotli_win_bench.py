#!/usr/bin/env python3
"""Rates of gpumt_brotli_compress_batch_win against gpumt_brotli_compress_batch_level on the bench text, device-resident: the
tables of profiles/brotli_win.txt.

  python tools/brotli_win_bench.py --mib 1024 --runs 3 [--levels 9,11] [--out file]
  python tools/brotli_win_bench.py --one win|level --mib 1024 --level 11 --chunk 0      one run (what rocprofv3 is given)

Every run is a process of its own under a time limit (a fault ends one run, not the job); the two calls alternate.  A run
generates the text, uploads it, encodes once untimed (first-use allocations) and once timed between two device events, and
prints milliseconds and the bytes written.  --chunk 0 = the quality's default chunk, 1 MiB x quality (include/brotli-mt.h)."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20260926                                            # bench.py's text


def one_run(call, mib, level, chunk):
    import ctypes as C
    import zstdmt_amd as z
    n = mib << 20
    t = C.CDLL(os.path.join(ROOT, "zstdmt_amd", "lib", "libzmt_tools.so"))
    t.zmt_gen_text.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int]
    text = np.empty(n, np.uint8)
    t.zmt_gen_text(text.ctypes.data, n, SEED, 0, 16)
    eng = z.Engine(0)
    d_in = eng.upload(text)
    nrec, stride = eng.record_count(n, chunk), eng.zstd_slot_stride(chunk)
    d_slots, d_len = eng.alloc(nrec * stride), eng.alloc(nrec * 4)
    ms = []
    for timed in (0, 1, 1):
        eng.timer_start(0)
        eng.brotli_compress(d_in, n, chunk, d_slots, stride, d_len, level=level, win=call == "win")
        eng.timer_stop(0)
        eng.sync(0)
        if timed:
            ms.append(eng.timer_ms(0))
    out = int(eng.download(d_len, nrec * 4, np.uint32).astype(np.uint64).sum())
    eng.close()
    print("ms %.2f %.2f bytes %d" % (ms[0], ms[1], out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--levels", default="9,11")
    ap.add_argument("--limit", type=int, default=240, help="seconds one run may take")
    ap.add_argument("--one")
    ap.add_argument("--level", type=int, default=11)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.one:
        return one_run(a.one, a.mib, a.level, a.chunk or a.level << 20)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%d MiB of the bench text, device-resident; per run two timed calls, the second one counted; GB/s of input" % a.mib)
    for level in (int(x) for x in a.levels.split(",")):
        for chunk in (level << 20, 1 << 20):
            res = {"level": [], "win": []}
            for _ in range(a.runs):
                for call in ("level", "win"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--one", call, "--mib", str(a.mib), "--level", str(level),
                           "--chunk", str(chunk)]
                    p = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd, capture_output=True, text=True)
                    w = p.stdout.split()
                    if p.returncode != 0 or len(w) != 5:
                        say("level %d chunk %d %s: run failed, rc %d: %s" % (level, chunk, call, p.returncode, p.stderr[-300:]))
                        return 1                             # nothing more is started on the device
                    res[call].append((float(w[2]), int(w[4])))
            for call in ("level", "win"):
                ms = sorted(r[0] for r in res[call])
                say("level %2d chunk %9d  %-5s  median %9.2f ms (%.2f .. %.2f)  %7.2f GB/s  ratio %.3f" % (
                    level, chunk, call, statistics.median(ms), ms[0], ms[-1], (a.mib << 20) / statistics.median(ms) / 1e6,
                    (a.mib << 20) / res[call][0][1]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
