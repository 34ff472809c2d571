#!/usr/bin/env python3
"""Rates of gpumt_lz4_decompress_batch (the baseline) and of gpumt_lz4_decompress_batch_par on the same device-resident
lz4-mt records, in one process: the table of profiles/lz4_rec_par.txt.

  python tools/lz4_rec_bench.py --mib 2048 --runs 5 [--out file]

The bench text, compressed on the device at each chunk size (blocks of 64 KiB: 2, 4, 8, 16, 64, 256 and 1024 blocks per
record), then decoded by: the baseline call; the new call on the par route; the new call on the seg route with segments of
64 KiB and of 16 KiB; and the par route once more with lz4_rec_slice_blocks at its maximum of 65536 (the other legs run
at the default of 4096 blocks per call of the block stages).  Two more rows decode records liblz4 wrote on the host
(--big-mib of the text): records of 16 MiB in blocks of 4 MiB (BD = 7), and records of 4 MiB in blocks of 64 KiB with
block checksums -- two of the kinds of record the baseline gives to one wave of zmt_lz4_dec_serial each.  Every leg is warmed once and timed --runs times with the handle's
event timers around the call; a leg's figure is the median, its spread is printed.  lz4_rec_min_blocks is 2 throughout, so
that every record of two blocks and more takes the route under test; the trace line of each leg's warm-up is printed in
its line.  Every frame carries a content checksum, which both calls verify: a leg whose statuses are not all OK ends the
job."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
CHUNKS = (128 << 10, 256 << 10, 512 << 10, 1 << 20, 4 << 20, 16 << 20, 64 << 20)
LEGS = (("baseline", None), ("par", dict(lz4_rec_seg=0)), ("seg_64k", dict(lz4_rec_seg=1, lz4_seg_bytes=65536)),
        ("seg_16k", dict(lz4_rec_seg=1, lz4_seg_bytes=16384)),
        ("par_slice64k", dict(lz4_rec_seg=0, lz4_rec_slice_blocks=65536)))


class Resident:
    """one stream on the device with everything a decode call needs"""

    def __init__(self, eng, d_stream, stream_bytes, rec_off, rec_len):
        self.eng, self.d_stream, self.stream_bytes, self.nrec = eng, d_stream, stream_bytes, len(rec_len)
        n = self.nrec
        self.d_ro, self.d_rl = eng.upload(np.asarray(rec_off, np.uint64)[:n].copy()), eng.upload(np.asarray(rec_len, np.uint32))
        self.d_ol, self.d_oo, self.d_st, self.d_rp = eng.alloc(n * 4), eng.alloc((n + 1) * 8), eng.alloc(n * 4), eng.alloc(n * 4)
        eng.lz4_probe(d_stream, self.d_ro, self.d_rl, n, self.d_ol, self.d_oo)
        self.total = int(eng.download(self.d_oo, (n + 1) * 8, np.uint64)[n])
        self.d_out = eng.alloc(self.total + 64)

    def free(self):
        for b in (self.d_stream, self.d_ro, self.d_rl, self.d_ol, self.d_oo, self.d_st, self.d_rp, self.d_out):
            b.free()

    def run(self, par):
        e = self.eng
        e.timer_start(0)
        if par:
            e.lz4_decompress_par(self.d_stream, self.stream_bytes, self.d_ro, self.d_rl, self.nrec, self.d_out, self.total,
                                 self.d_oo, self.d_ol, self.d_st, self.d_rp)
        else:
            e.lz4_decompress(self.d_stream, self.stream_bytes, self.d_ro, self.d_rl, self.nrec, self.d_out, self.total,
                             self.d_oo, self.d_ol, self.d_st)
        e.timer_stop(0)
        e.sync()
        return e.timer_ms(0)

    def statuses_ok(self):
        return not self.eng.download(self.d_st, self.nrec * 4, np.uint32).any()


def device_stream(eng, d_in, n, chunk):
    nrec = eng.record_count(n, chunk)
    stride = eng.slot_stride(chunk)
    d_slots, d_len, d_off = eng.alloc(nrec * stride), eng.alloc(nrec * 4), eng.alloc((nrec + 1) * 8)
    try:
        eng.lz4_compress(d_in, n, chunk, d_slots, stride, d_len)
        rec_len = eng.download(d_len, nrec * 4, np.uint32)
        total = int(rec_len.astype(np.uint64).sum())
        d_stream = eng.alloc(total + 320)
        eng.lz4_compact(d_slots, stride, d_len, nrec, d_stream, d_off)
        rec_off = eng.download(d_off, (nrec + 1) * 8, np.uint64)
    finally:
        for b in (d_slots, d_len, d_off):
            b.free()
    return Resident(eng, d_stream, total, rec_off, rec_len)


def host_stream(eng, data, rec_bytes, **prefs):
    """records of rec_bytes in linked blocks, written by liblz4 with `prefs` -> Resident, or None without liblz4"""
    import helpers as H
    recs = []
    for i in range(0, len(data), rec_bytes):
        fr = H.liblz4_frame(data[i:i + rec_bytes], linked=1, content_size=1, checksum=1, **prefs)
        if fr is None:
            return None
        recs.append(H.mt_record(fr))
    stream = b"".join(recs)
    rec_len = np.array([len(r) for r in recs], np.uint32)
    rec_off = np.concatenate(([0], np.cumsum(rec_len.astype(np.uint64)))).astype(np.uint64)
    return Resident(eng, eng.upload(stream, slack=320), len(stream), rec_off, rec_len)


def legs(a, say, eng, K, res, name):
    say("\n## %s: %d records, %d -> %d bytes" % (name, res.nrec, res.stream_bytes, res.total))
    medians = {}
    for leg, knobs in LEGS:
        prev = {k: eng.set_variant(k, v) for k, v in (knobs or {}).items()}
        lines = []
        try:
            with K.captured_stderr(lines):
                res.run(knobs is not None)                      # the warm-up: scratch is allocated here
            if not res.statuses_ok():
                say("%s: a record failed; the job ends here" % leg)
                return None
            ms = sorted(res.run(knobs is not None) for _ in range(a.runs))
        finally:
            for k, v in prev.items():
                eng.set_variant(k, v)
        tr = K.trace_stats(lines)
        med = ms[len(ms) // 2]
        medians[leg] = med
        say("%-12s median %8.3f ms = %7.2f GB/s  (spread %.3f-%.3f ms, %d runs)  %s" % (
            leg, med, res.total / med / 1e6, ms[0], ms[-1], len(ms),
            " ".join("%s %s" % kv for kv in tr[0].items()) if tr else ""))
    say("=> time against the baseline (below 1 = faster): " +
        ", ".join("%s %.3f" % (leg, medians[leg] / medians["baseline"]) for leg, _ in LEGS[1:]))
    return medians


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=2048)
    ap.add_argument("--big-mib", type=int, default=256, help="MiB of the 4 MiB-block stream (written on the host)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5, "the median of at least 5 timed repeats"
    import lz4_rec as K
    import zstdmt_amd as z
    from golden import cases
    out = open(a.out, "a") if a.out else sys.stdout

    def say(*x):
        print(*x, file=out, flush=True)
    n = a.mib << 20
    data = cases.text(n)
    old = os.environ.get("GPUMT_TRACE")
    os.environ["GPUMT_TRACE"] = "1"
    eng = z.Engine(0)
    if old is None:
        del os.environ["GPUMT_TRACE"]
    say("# %s; %d MiB of the bench text, device-resident; event timers around the call; %d timed runs per leg after one"
        " warm-up; lz4_rec_min_blocks 2" % (eng.name, a.mib, a.runs))
    assert eng.set_variant("lz4_rec_min_blocks", 2) != -1
    d_in = eng.upload(data)
    try:
        for chunk in CHUNKS:
            res = device_stream(eng, d_in, n, chunk)
            try:
                if legs(a, say, eng, K, res, "chunk %d KiB, %d blocks of 64 KiB per record" % (chunk >> 10, chunk >> 16)) is None:
                    return 1
            finally:
                res.free()
    finally:
        d_in.free()
    for name, rec_bytes, prefs in (("records of 16 MiB in 4 blocks of 4 MiB (BD = 7, liblz4)", 16 << 20, dict(block_id=7)),
                                   ("records of 4 MiB in 64 blocks of 64 KiB with block checksums (liblz4)", 4 << 20,
                                    dict(block_id=4, block_checksum=1))):
        big = host_stream(eng, data[:a.big_mib << 20], rec_bytes, **prefs)
        if big is None:
            say("\n## %s: no liblz4 on this machine, row missing" % name)
            continue
        try:
            if legs(a, say, eng, K, big, name) is None:
                return 1
        finally:
            big.free()
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
