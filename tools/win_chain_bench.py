#!/usr/bin/env python3
"""The window encoders with their chain plane built by one wave per chunk ("win_chain_par" 0) and in segments (seg_log 16,
18, 20), on the bench text, device-resident: the table of profiles/win_chain_par.txt.

  python tools/win_chain_bench.py --mib 1024 --runs 3 [--rows zstd:10:8388608,...] [--segs 0,16,18,20] [--out file]
  python tools/win_chain_bench.py --one zstd --mib 1024 --level 19 --chunk 67108864 --seg 18      one run (what rocprofv3 is given)

Every run is a process of its own under a time limit (a fault ends one run, not the job); within a row the settings alternate,
so that a drift of the device meets all of them.  A run generates the text, uploads it, encodes once untimed (first-use
allocations) and twice timed between two device events, the second one counted, and prints milliseconds, the bytes written
and the head-table bytes of the segment build."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20260926                                            # bench.py's text
ROWS = "zstd:10:8388608,zstd:10:1048576,zstd:19:67108864,zstd:19:1048576,brotli:11:11534336"
SLICE = 1 << 30                                            # the _win calls' launch slice


def one_run(codec, mib, level, chunk, seg):
    import ctypes as C
    import zstdmt_amd as z
    n = mib << 20
    t = C.CDLL(os.path.join(ROOT, "zstdmt_amd", "lib", "libzmt_tools.so"))
    t.zmt_gen_text.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int]
    text = np.empty(n, np.uint8)
    t.zmt_gen_text(text.ctypes.data, n, SEED, 0, 16)
    eng = z.Engine(0)
    if eng.set_variant("win_chain_par", seg) < 0:
        return 2
    d_in = eng.upload(text)
    nrec, stride = eng.record_count(n, chunk), eng.zstd_slot_stride(chunk)
    d_slots, d_len = eng.alloc(nrec * stride), eng.alloc(nrec * 4)
    call = eng.zstd_compress if codec == "zstd" else eng.brotli_compress
    ms = []
    for timed in (0, 1, 1):
        eng.timer_start(0)
        call(d_in, n, chunk, d_slots, stride, d_len, level=level, win=True)
        eng.timer_stop(0)
        eng.sync(0)
        if timed:
            ms.append(eng.timer_ms(0))
    out = int(eng.download(d_len, nrec * 4, np.uint32).astype(np.uint64).sum())
    heads = eng.win_chain_par_scratch(min(n, SLICE // chunk * chunk), chunk, seg) if seg else 0
    eng.close()
    print("ms %.2f %.2f bytes %d heads %d" % (ms[0], ms[1], out, heads))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", default=ROWS, help="codec:level:chunk, comma separated")
    ap.add_argument("--segs", default="0,16,18,20", help="win_chain_par settings; 0 = one wave per chunk")
    ap.add_argument("--limit", type=int, default=120, help="seconds one run may take")
    ap.add_argument("--one")
    ap.add_argument("--level", type=int, default=19)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.one:
        return one_run(a.one, a.mib, a.level, a.chunk, a.seg)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                          # kept as it grows: a job that is cut short leaves what it had
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    segs = [int(x) for x in a.segs.split(",")]
    say("%d MiB of the bench text, device-resident; per run one untimed and two timed calls, the second one counted; "
        "medians of %d (min .. max); GB/s of input" % (a.mib, a.runs))
    for row in a.rows.split(","):
        codec, level, chunk = row.split(":")[0], int(row.split(":")[1]), int(row.split(":")[2])
        res = {s: [] for s in segs}
        for _ in range(a.runs):
            for s in segs:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", codec, "--mib", str(a.mib), "--level", str(level),
                       "--chunk", str(chunk), "--seg", str(s)]
                p = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd, capture_output=True, text=True)
                w = p.stdout.split()
                if p.returncode != 0 or len(w) != 7:
                    say("%s level %d chunk %d seg_log %d: run failed, rc %d: %s" % (codec, level, chunk, s, p.returncode,
                                                                                   p.stderr[-300:]))
                    return 1                               # nothing more is started on the device
                res[s].append((float(w[2]), int(w[4]), int(w[6])))
        off_min = min(r[0] for r in res[segs[0]])
        for s in segs:
            ms = sorted(r[0] for r in res[s])
            med = statistics.median(ms)
            same = all(r[1] == res[segs[0]][0][1] for r in res[s])
            say("%-6s level %2d chunk %9d  seg_log %2d  median %9.2f ms (%.2f .. %.2f)  %6.2f GB/s  heads %11d  bytes %s  %s" % (
                codec, level, chunk, s, med, ms[0], ms[-1], (a.mib << 20) / med / 1e6, res[s][0][2],
                "same" if same else "DIFFER", "" if s == segs[0] else "below the off minimum" if med < off_min else "not below"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
