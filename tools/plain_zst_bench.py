#!/usr/bin/env python3
"""Rates of ZSTDCB_decompressDCtx on plain .zst input (one frame per stream, memcpy callbacks), one library against
another on the same streams: the tables of profiles/plain_zst_blocks.txt.

  python tools/plain_zst_bench.py --mib 256 --runs 3 --old path/to/parent/libzstdmt_amd.so [--new path] [--out file]
  python tools/plain_zst_bench.py --rss-mib 1024 --old ...      peak host RSS of one decode, either library
  python tools/plain_zst_bench.py --rle-blocks 16400            the hand-built frame of RLE blocks above 2 GiB (new only)
  python tools/plain_zst_bench.py --small-mib 256 --old ...     the same text as frames of 192 KiB, one behind the other
  python tools/plain_zst_bench.py --stages --mib 256 --old ...  three legs per input instead of two: the old library with
      nothing set (serial call) and under GPUMT_ZSTD_RUN_PRE=1 (pre call), the new one under GPUMT_ZSTD_RUN_PAR=1 (par call);
      with --small-mib likewise

Every run is a process of its own (a library reads its batch size once; a fault ends one run, not the job) under a time
limit; the two libraries alternate.  The callbacks copy up to 128 KiB per call, the library's piece size.  GPUMT_TRACE=1
is set for the new library: its per-stage times go into the output."""
import argparse
import ctypes as C
import os
import resource
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)

STREAMS = [("level3_no_checksum", dict(level=3, checksum=0)), ("level3_checksum", dict(level=3, checksum=1))]


def one_run(libpath, path, nout, keep):
    """child: decode the stream once -> prints seconds, a checksum of the output (or its zero count) and the peak RSS"""
    import helpers as H
    lib = H.bind_lz4mt(C.CDLL(libpath), "ZSTDCB_")
    with open(path, "rb") as f:
        st = f.read()
    src = C.create_string_buffer(st, len(st))
    dst = C.create_string_buffer(nout + 64 if keep else 1)
    pos = [0, 0, 0]

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
        if keep:
            C.memmove(C.addressof(dst) + pos[1], b.buf, b.size)
        else:
            pos[2] += b.size - C.string_at(b.buf, b.size).count(0)
        pos[1] += b.size
        return 0
    io = H.RefRdWr(H.RD_FN(rd), None, H.RD_FN(wr), None)
    ctx = lib.ZSTDCB_createDCtx(4, 0)
    t0 = time.perf_counter()
    rv = lib.ZSTDCB_decompressDCtx(ctx, C.byref(io))
    dt = time.perf_counter() - t0
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss // 1024
    lib.ZSTDCB_freeDCtx(ctx)
    if rv != 0 or pos[1] != nout:
        print("FAILED rv=%d (%s) out=%d" % (C.c_ssize_t(rv).value, lib.ZSTDCB_getErrorString(rv), pos[1]))
        return 1
    if keep:
        import xxhash
        print("seconds %.4f rss_mib %d xxh %08x" % (dt, rss, xxhash.xxh32(dst.raw[:nout], seed=0).intdigest()))
    else:
        print("seconds %.4f rss_mib %d nonzero %d" % (dt, rss, pos[2]))
    return 0


def child(a, libpath, path, n, keep, trace, extra=None):
    env = dict(os.environ)
    if extra is not None: # a leg of --stages: the two variables are the leg's own
        env.pop("GPUMT_ZSTD_RUN_PRE", None)
        env.pop("GPUMT_ZSTD_RUN_PAR", None)
        env.update(extra)
    if trace:
        env["GPUMT_TRACE"] = "1"
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", libpath, path, str(n), str(int(keep))],
                           capture_output=True, text=True, timeout=a.limit, env=env)
    except subprocess.TimeoutExpired:
        return None, "no result within %d s" % a.limit, []
    line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else "(no output)"
    if p.returncode != 0 or not line.startswith("seconds"):
        return None, "exit %d %s %s" % (p.returncode, line, p.stderr[-300:]), []
    return float(line.split()[1]), line, [t.strip() for t in p.stderr.splitlines() if "[zstdmt plain" in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=0)
    ap.add_argument("--rss-mib", type=int, default=0)
    ap.add_argument("--rle-blocks", type=int, default=0)
    ap.add_argument("--small-mib", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--old", default=None)
    ap.add_argument("--new", default=os.path.join(ROOT, "zstdmt_amd", "lib", "libzstdmt_amd.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per run")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--child", nargs=4)
    a = ap.parse_args()
    if a.child:
        sys.exit(one_run(a.child[0], a.child[1], int(a.child[2]), int(a.child[3])))
    import helpers as H
    from golden import cases
    out = open(a.out, "a") if a.out else sys.stdout

    def say(*x):
        print(*x, file=out, flush=True)
    libs = ([("old", a.old, None)] if a.old else []) + [("new", a.new, None)]
    if a.stages:
        assert a.old, "--stages compares against the parent's library"
        libs = [("old_serial", a.old, {}), ("old_pre", a.old, {"GPUMT_ZSTD_RUN_PRE": "1"}),
                ("new_par", a.new, {"GPUMT_ZSTD_RUN_PAR": "1"})]
    say("# old = %s\n# new = %s" % (a.old, a.new))
    if a.mib or a.small_mib:
        n = (a.mib or a.small_mib) << 20
        data = cases.text(n)
        small = 192 << 10  # many frames side by side: 1.5 blocks each, every frame a run of its own
        say("# ZSTDCB_decompressDCtx, plain .zst, %s of %d MiB of the bench text, memcpy callbacks"
            % ("one frame" if a.mib else "frames of %d KiB" % (small >> 10), n >> 20))
        say("# %d runs each, the legs alternating; GB/s of content" % a.runs)
        for name, kw in (STREAMS if a.mib else [("small_frames_level3", dict(level=3, checksum=0))]):
            path = os.path.join(a.tmp, "plain_%s.zst" % name)
            if a.mib:
                fr = H.libzstd_frame(data, **kw)
            else:
                fr = b"".join(H.libzstd_frame(data[i:i + small], **kw) for i in range(0, n, small))
            with open(path, "wb") as f:
                f.write(fr)
            say("\n## %s: %d -> %d bytes" % (name, len(fr), n))
            rates = {which: [] for which, _, _ in libs}
            for r in range(a.runs):
                for which, libpath, extra in libs:
                    sec, line, trace = child(a, libpath, path, n, True, which.startswith("new"), extra)
                    if sec is None:
                        say("%s run %d: %s; the job ends here" % (which, r, line))
                        return 1
                    rates[which].append(n / sec / 1e9)
                    say("%s run %d: %.3f s = %.3f GB/s  %s" % (which, r, sec, n / sec / 1e9, " ".join(line.split()[2:])))
                    for t in trace:
                        say("    " + t)
            for which, _, _ in libs:
                v = sorted(rates[which])
                say("=> %s median %.4f GB/s (spread %.4f-%.4f)" % (which, v[len(v) // 2], v[0], v[-1]))
            os.unlink(path)
    if a.rss_mib:
        n = a.rss_mib << 20
        path = os.path.join(a.tmp, "plain_rss.zst")
        unit = cases.text(64 << 20)
        with open(path, "wb") as f:
            f.write(H.libzstd_frame(unit * (n // len(unit)), level=1, checksum=0))
        say("\n## peak host RSS, one frame of %d MiB (64 MiB of the bench text repeated, level 1), output counted, not kept"
            % a.rss_mib)
        for which, libpath, extra in libs:
            sec, line, trace = child(a, libpath, path, n, False, which.startswith("new"), extra)
            say("%s: %s" % (which, line))
            for t in trace:
                say("    " + t)
            if sec is None:
                return 1
        os.unlink(path)
    if a.rle_blocks:
        nb, n = a.rle_blocks, a.rle_blocks * 131072
        fr = bytearray(bytes([0x28, 0xB5, 0x2F, 0xFD, 3 << 6, 7 << 3]) + struct.pack("<Q", n))
        fr += ((1 << 1 | 131072 << 3).to_bytes(3, "little") + b"\0") * (nb - 1)
        fr += (1 | 1 << 1 | 131072 << 3).to_bytes(3, "little") + b"\0"
        path = os.path.join(a.tmp, "plain_rle.zst")
        with open(path, "wb") as f:
            f.write(fr)
        say("\n## %d RLE blocks of 128 KiB behind an 8-byte content size: %d -> %d bytes, output counted, not kept"
            % (nb, len(fr), n))
        for r in range(a.runs):
            sec, line, trace = child(a, a.new, path, n, False, True)
            if sec is None:
                say("new run %d: %s; the job ends here" % (r, line))
                return 1
            say("new run %d: %.3f s = %.3f GB/s  %s" % (r, sec, n / sec / 1e9, " ".join(line.split()[2:])))
            for t in trace:
                say("    " + t)
        os.unlink(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
