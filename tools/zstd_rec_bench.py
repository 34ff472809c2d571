#!/usr/bin/env python3
"""Rates of ZSTDCB_decompressDCtx on zstd-mt streams the reference build wrote (oracle/_ref), the parent's library with
nothing set against this library under GPUMT_ZSTD_REC_PAR=1: the tables of profiles/zstd_rec_par.txt.

  python tools/zstd_rec_bench.py --mib 1024 --runs 3 --old path/to/parent/libzstdmt_amd.so [--new path] [--out file]
  python tools/zstd_rec_bench.py --mib 1024 --sweep --old ...     also zstd_rec_min_blocks 2 / 4 / 8 / 16 on the 2 MiB stream

Three streams of the bench text at level 3: the reference's default chunk (2 MiB, 16 blocks per record), inputsize 64 MiB
(512 blocks per record) and inputsize 128 KiB (one block per record: the control, where no record is eligible).  Every
run is a process of its own under a time limit (tools/plain_zst_bench.py's child: the whole call is timed, memcpy
callbacks), the legs alternate, and a run that fails or runs out of time ends the job.  GPUMT_TRACE=1 is set for the new
library: the `[gpumt zstd rec]` lines of a run are summed into its line."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
PLAIN = os.path.join(ROOT, "tools", "plain_zst_bench.py")
STREAMS = [("level3_chunk_2m", 0), ("level3_chunk_64m", 64 << 20), ("level3_chunk_128k", 128 << 10)]
VARS = ("GPUMT_ZSTD_REC_PAR", "GPUMT_ZSTD_REC_MIN_BLOCKS", "GPUMT_ZSTD_REC_SLICE_BLOCKS")


def child(a, libpath, path, n, extra):
    """one decode in a process of its own -> (seconds or None, the child's line, summed trace figures)"""
    env = dict(os.environ, GPUMT_TRACE="1")
    for k in VARS:
        env.pop(k, None)
    env.update(extra)
    try:
        p = subprocess.run([sys.executable, PLAIN, "--child", libpath, path, str(n), "1"], capture_output=True, text=True,
                           timeout=a.limit, env=env)
    except subprocess.TimeoutExpired:
        return None, "no result within %d s" % a.limit, {}
    line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else "(no output)"
    if p.returncode != 0 or not line.startswith("seconds"):
        return None, "exit %d %s %s" % (p.returncode, line, p.stderr[-300:]), {}
    tr = {}
    for t in p.stderr.splitlines():
        if t.startswith("[gpumt zstd rec]"):
            w = t.split()
            tr["calls"] = tr.get("calls", 0) + 1
            for i in range(3, 13, 2):
                tr[w[i]] = tr.get(w[i], 0) + int(w[i + 1])
    return float(line.split()[1]), line, tr


def legs(a, say, path, n, libs):
    rates = {which: [] for which, _, _ in libs}
    for r in range(a.runs):
        for which, libpath, extra in libs:
            sec, line, tr = child(a, libpath, path, n, extra)
            if sec is None:
                say("%s run %d: %s; the job ends here" % (which, r, line))
                return False
            rates[which].append(n / sec / 1e9)
            say("%s run %d: %.3f s = %.3f GB/s  %s  %s" % (which, r, sec, n / sec / 1e9, " ".join(line.split()[2:]),
                                                        " ".join("%s %d" % kv for kv in tr.items())))
    for which, _, _ in libs:
        v = sorted(rates[which])
        say("=> %s median %.4f GB/s (spread %.4f-%.4f)" % (which, v[len(v) // 2], v[0], v[-1]))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "zstdmt_amd", "lib", "libzstdmt_amd.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds per run")
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    import helpers as H
    from golden import cases
    assert H.have_zref(), "the reference build (oracle/_ref) writes the streams"
    out = open(a.out, "a") if a.out else sys.stdout

    def say(*x):
        print(*x, file=out, flush=True)
    n = a.mib << 20
    data = cases.text(n)
    say("# old = %s (nothing set)\n# new = %s (GPUMT_ZSTD_REC_PAR=1)" % (a.old, a.new))
    say("# ZSTDCB_decompressDCtx, zstd-mt records written by the reference build at level 3, %d MiB of the bench text,"
        " memcpy callbacks\n# %d runs each, the legs alternating; GB/s of content" % (a.mib, a.runs))
    libs = [("old", a.old, {}), ("new_rec_par", a.new, {"GPUMT_ZSTD_REC_PAR": "1"})]
    for name, inputsize in STREAMS:
        path = os.path.join(a.tmp, "rec_%s.zstdmt" % name)
        rv, st, _, stats = H.zstdmt_compress_via(H.zref(), data, inputsize, threads=4, level=3)
        assert rv == 0
        with open(path, "wb") as f:
            f.write(st)
        say("\n## %s: %d records, %d -> %d bytes" % (name, stats[0], len(st), n))
        del st
        ok = legs(a, say, path, n, libs)
        if ok and a.sweep and inputsize == 0:
            say("\n## %s, zstd_rec_min_blocks sweep (new library, GPUMT_ZSTD_REC_PAR=1)" % name)
            ok = legs(a, say, path, n, [("min_blocks_%d" % m, a.new, {"GPUMT_ZSTD_REC_PAR": "1",
                                                                     "GPUMT_ZSTD_REC_MIN_BLOCKS": str(m)}) for m in (2, 4, 8, 16)])
        os.unlink(path)
        if not ok:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
