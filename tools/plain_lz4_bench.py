#!/usr/bin/env python3
"""Rates of LZ4MT_decompressDCtx on plain .lz4 input (one frame per stream, memcpy callbacks), one library against
another on the same streams: the table of profiles/plain_lz4_blocks.txt.

  python tools/plain_lz4_bench.py --mib 1024 --runs 3 --old path/to/parent/libzstdmt_amd.so [--new path] [--out file]

Every run is a process of its own (a library reads its batch size once; a fault ends one run, not the job) under a time
limit; the two libraries alternate (both see the caller's environment, GPUMT_LZ4_RUN_PAR and GPUMT_LZ4_BLOCK_SEG included: a
library that does not know a variable ignores it).  --legs name,name runs only those streams.  The callbacks copy 4 MiB per
call, so the interpreter's share is a few hundred calls per GiB.  GPUMT_TRACE=1 is set for the new library: its per-stage times go into the output."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)

STREAMS = [  # name, liblz4_frame arguments
    ("4MiB_independent_nochecksum", dict(block_id=7, linked=0, checksum=0)),
    ("4MiB_independent_checksum", dict(block_id=7, linked=0, checksum=1)),
    ("4MiB_linked_checksum", dict(block_id=7, linked=1, checksum=1)),
    ("64KiB_independent_checksum", dict(block_id=4, linked=0, checksum=1)),
    ("64KiB_linked_checksum", dict(block_id=4, linked=1, checksum=1)),  # the LZ4F library default
]


def one_run(libpath, path, nout):
    """child: decode the stream once -> prints seconds"""
    import helpers as H
    lib = H.bind_lz4mt(C.CDLL(libpath))
    with open(path, "rb") as f:
        st = f.read()
    src = C.create_string_buffer(st, len(st))
    dst = C.create_string_buffer(nout + 64)
    pos = [0, 0]

    def rd(_a, bp):
        b = bp.contents
        n = min(b.size, len(st) - pos[0])
        C.memmove(b.buf, C.addressof(src) + pos[0], n)
        pos[0] += n
        b.size = n
        return 0

    def wr(_a, bp):
        b = bp.contents
        if pos[1] + b.size > nout:
            return -1
        C.memmove(C.addressof(dst) + pos[1], b.buf, b.size)
        pos[1] += b.size
        return 0
    io = H.RefRdWr(H.RD_FN(rd), None, H.RD_FN(wr), None)
    ctx = lib.LZ4MT_createDCtx(4, 4 << 20)
    t0 = time.perf_counter()
    rv = lib.LZ4MT_decompressDCtx(ctx, C.byref(io))
    dt = time.perf_counter() - t0
    lib.LZ4MT_freeDCtx(ctx)
    if rv != 0 or pos[1] != nout:
        print("FAILED rv=%d out=%d" % (rv, pos[1]))
        return 1
    import xxhash
    print("seconds %.4f xxh %08x" % (dt, xxhash.xxh32(dst.raw[:nout], seed=0).intdigest()))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "zstdmt_amd", "lib", "libzstdmt_amd.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per run")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--legs", default=None, help="comma-separated stream names (default: all)")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        sys.exit(one_run(a.child[0], a.child[1], int(a.child[2])))
    import helpers as H
    from golden import cases
    out = open(a.out, "w") if a.out else sys.stdout

    def say(*x):
        print(*x, file=out, flush=True)
    n = a.mib << 20
    data = cases.text(n)
    say("# LZ4MT_decompressDCtx, plain .lz4, one frame of %d MiB of the bench text, memcpy callbacks (4 MiB requests)" % a.mib)
    say("# old = %s\n# new = %s\n# %d runs each, alternating old / new; GB/s of content" % (a.old, a.new, a.runs))
    legs = a.legs.split(",") if a.legs else [name for name, _ in STREAMS]
    assert all(leg in dict(STREAMS) for leg in legs), legs
    for name, kw in STREAMS:
        if name not in legs:
            continue
        path = os.path.join(a.tmp, "plain_%s.lz4" % name)
        with open(path, "wb") as f:
            fr = H.liblz4_frame(data, content_size=0, **kw)
            f.write(fr)
        say("\n## %s: %d -> %d bytes" % (name, len(fr), n))
        rates = {"old": [], "new": []}
        for r in range(a.runs):
            for which, libpath in (("old", a.old), ("new", a.new)):
                env = dict(os.environ)
                if which == "new":
                    env["GPUMT_TRACE"] = "1"
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--old", a.old, "--child", libpath, path,
                                        str(n)], capture_output=True, text=True, timeout=a.limit, env=env)
                except subprocess.TimeoutExpired:
                    say("%s run %d: no result within %d s; the job ends here" % (which, r, a.limit))
                    return 1
                line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else "(no output)"
                if p.returncode != 0 or not line.startswith("seconds"):
                    say("%s run %d: exit %d %s %s; the job ends here" % (which, r, p.returncode, line, p.stderr[-300:]))
                    return 1
                sec = float(line.split()[1])
                rates[which].append(n / sec / 1e9)
                say("%s run %d: %.3f s = %.3f GB/s  %s" % (which, r, sec, n / sec / 1e9, line.split()[-1]))
                for t in p.stderr.splitlines():
                    if "[lz4mt plain" in t:
                        say("    " + t.strip())
        o, w = sorted(rates["old"]), sorted(rates["new"])
        say("=> old median %.3f GB/s (spread %.3f-%.3f), new median %.3f GB/s (spread %.3f-%.3f), new / old = %.2f"
            % (o[len(o) // 2], o[0], o[-1], w[len(w) // 2], w[0], w[-1], w[len(w) // 2] / o[len(o) // 2]))
        os.unlink(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
