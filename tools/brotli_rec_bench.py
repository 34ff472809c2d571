#!/usr/bin/env python3
"""Rates of gpumt_brotli_decompress_batch (serial) and of gpumt_brotli_decompress_batch_par on the same device-resident
brotli-mt records, in one process: the table of profiles/brotli_rec_par.txt.

  python tools/brotli_rec_bench.py --mib 1024 --runs 5 [--out file]

The bench text, compressed on the device with gpumt_brotli_compress_batch_index at chunks of 1, 4 and 9 MiB (qualities 1,
4 and 9: the reference's default chunk is 1 MiB x level) and at 128 KiB, where a record is one block, has no index and the
new call reduces to the serial one.  Per configuration: the index's size cost against gpumt_brotli_compress_batch_level,
one warm-up of each call (scratch is allocated there; its trace line is printed), then --runs timed repeats of each with
the handle's event timers, serial and par interleaved, medians and spreads.  brotli_rec_min_spans is 2 throughout.  A
configuration whose statuses are not all OK, or whose outputs differ between the two calls, ends the job."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
CONFIGS = ((1 << 20, 1), (4 << 20, 4), (9 << 20, 9), (128 << 10, 1))


def device_stream(eng, d_in, n, chunk, level, index):
    """-> (d_stream, rec_off of the payloads, rec_len of the payloads, capacities, stream bytes)"""
    nrec = eng.record_count(n, chunk)
    stride = eng.zstd_slot_stride(chunk)
    d_slots, d_len, d_off = eng.alloc(nrec * stride), eng.alloc(nrec * 4), eng.alloc((nrec + 1) * 8)
    try:
        eng.brotli_compress(d_in, n, chunk, d_slots, stride, d_len, level=level, index=index)
        rec_len = eng.download(d_len, nrec * 4, np.uint32)
        total = int(rec_len.astype(np.uint64).sum())
        d_stream = eng.alloc(total + 320)
        eng.lz4_compact(d_slots, stride, d_len, nrec, d_stream, d_off)
        rec_off = eng.download(d_off, (nrec + 1) * 8, np.uint64)[:nrec]
    finally:
        for b in (d_slots, d_len, d_off):
            b.free()
    sizes = np.minimum(chunk, n - np.arange(nrec, dtype=np.uint64) * chunk)
    cap = (((sizes + 65535) >> 16) << 16).astype(np.uint32)        # at least the hint's 64 KiB units
    return d_stream, rec_off + 16, rec_len - 16, cap, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5, "the median of at least 5 timed repeats"
    import brotli_rec as R
    import zstdmt_amd as z
    from golden import cases
    out = open(a.out, "a") if a.out else sys.stdout

    def say(*x):
        print(*x, file=out, flush=True)
    n = a.mib << 20
    os.environ["GPUMT_TRACE"] = "1"
    eng = z.Engine(0)
    say("# brotli_rec_bench: %d MiB of the bench text on %s, %d timed repeats per call, interleaved" % (a.mib, eng.name, a.runs))
    d_in = eng.upload(cases.text(n))
    try:
        for chunk, level in CONFIGS:
            d_plain, _, plain_len, _, plain_total = device_stream(eng, d_in, n, chunk, level, False)
            d_plain.free()
            d_stream, ro, rl, cap, total = device_stream(eng, d_in, n, chunk, level, True)
            nrec = len(rl)
            oo = np.zeros(nrec, np.uint64)
            oo[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
            bufs = [eng.upload(ro.astype(np.uint64)), eng.upload(rl.astype(np.uint32)), eng.upload(oo), eng.upload(cap)]
            d_ol, d_st, d_rp = eng.alloc(nrec * 4), eng.alloc(nrec * 4), eng.alloc(nrec * 4)
            outs = [eng.alloc(int(oo[-1]) + int(cap[-1]) + 64) for _ in range(2)]
            say("\n## chunk %d KiB, quality %d: %d records, %d -> %d bytes; the index costs %d bytes (%.4f %%), %.1f per record" % (
                chunk >> 10, level, nrec, n, total, total - plain_total, 100.0 * (total - plain_total) / plain_total,
                (total - plain_total) / nrec))

            def run(par):
                eng.timer_start(0)
                if par:
                    eng.brotli_decompress_par(d_stream, bufs[0], bufs[1], nrec, outs[1], bufs[2], bufs[3], d_ol, d_st, d_rp)
                else:
                    eng.brotli_decompress(d_stream, bufs[0], bufs[1], nrec, outs[0], bufs[2], bufs[3], d_ol, d_st)
                eng.timer_stop(0)
                eng.sync()
                return eng.timer_ms(0)
            ok, lines = True, []
            for par in (False, True):
                with R.captured_stderr(lines):
                    run(par)
                ok = ok and not eng.download(d_st, nrec * 4, np.uint32).any()
            same = all((eng.download(outs[0], int(c), offset=int(o)) == eng.download(outs[1], int(c), offset=int(o))).all()
                       for o, c in list(zip(oo, np.minimum(cap, 1 << 20)))[:64])
            if not ok or not same:
                say("a record failed or the outputs differ; the job ends here")
                return 1
            ms = {False: [], True: []}
            for _ in range(a.runs):
                for par in (False, True):
                    ms[par].append(run(par))
            tr = R.trace_stats(lines)
            for par, name in ((False, "serial"), (True, "par")):
                v = sorted(ms[par])
                say("%-7s median %9.3f ms = %7.2f GB/s  (spread %.3f-%.3f ms)  %s" % (
                    name, v[len(v) // 2], n / v[len(v) // 2] / 1e6, v[0], v[-1],
                    " ".join("%s %s" % kv for kv in tr[0].items()) if par and tr else ""))
            say("=> par / serial: %.3f (below 1 = faster)" % (sorted(ms[True])[a.runs // 2] / sorted(ms[False])[a.runs // 2]))
            for b in bufs + outs + [d_stream, d_ol, d_st, d_rp]:
                b.free()
    finally:
        d_in.free()
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
