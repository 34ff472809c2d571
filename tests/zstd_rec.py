"""Helpers of the block-parallel record path tests (TEST CODE ONLY): batches of zstd-mt records through
gpumt_zstd_decompress_batch_par and through gpumt_zstd_decompress_batch, on the emulator and on the device, and the cases
that tests/test_emu_zstd_rec_par.py and tests/test_gpu_zstd_rec_par.py share.  A record is 12 bytes of
50 2A 4D 18 | 04 00 00 00 | csize followed by the frame."""
import contextlib
import ctypes as C
import functools
import os
import struct
import tempfile

import numpy as np

import emu_driver as E
import helpers as H
import zstd_blocks as Z
import zstd_par as R
import zstd_pre as P
import zstd_synth as S

CANARY = 0xCC
GAP = 7            # canary bytes between two records' output ranges (odd: the ranges start at every alignment)
JUNK = b"\xEE" * 3  # bytes between two records of the stream, which belong to no record
ST_BAD_CHECKSUM = 5
KNOBS = dict(min_blocks=1, slice_blocks=4096, rec_par=1, cap_mb=0)
GOLDEN_MT = os.path.join(H.GOLDEN_DIR, "zstd")


class Batch:
    """records = [(record bytes, out_len on entry (content size or capacity), status on entry)]"""

    def __init__(self, records):
        self.records = [(bytes(r), int(c), int(s)) for r, c, s in records]
        n = len(self.records)
        self.rec_off, self.rec_len = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self.out_off, self.cap = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self.status = np.array([s for _, _, s in self.records], np.uint32)
        stream, at = bytearray(JUNK), GAP
        for i, (r, c, _) in enumerate(self.records):
            self.rec_off[i], self.rec_len[i] = len(stream), len(r)
            stream += r + JUNK
            self.out_off[i], self.cap[i] = at, c
            at += c + GAP
        self.stream, self.out_bytes = bytes(stream), at

    def __len__(self):
        return len(self.records)


class Result:
    def __init__(self, batch, area, out_len, status, rec_par=None, stats=None):
        self.batch, self.area, self.out_len, self.status = batch, area, out_len, status
        self.rec_par, self.stats = rec_par, stats

    def bytes_of(self, i, n=None):
        o = int(self.batch.out_off[i])
        return self.area[o:o + int(self.out_len[i] if n is None else n)].tobytes()

    def gaps_intact(self):
        """every byte outside the records' [out_off, out_off + cap) still holds the canary"""
        keep = np.ones(len(self.area), bool)
        for o, c in zip(self.batch.out_off, self.batch.cap):
            keep[int(o):int(o) + int(c)] = False
        return bool((self.area[keep] == CANARY).all())


def _arrays(b):
    sbuf = np.frombuffer(b.stream + b"\xEE" * 320, np.uint8).copy()       # the device contract: 256 readable bytes behind
    area = np.full(b.out_bytes + 64, CANARY, np.uint8)
    return sbuf, area, b.rec_off.copy(), b.rec_len.copy(), b.out_off.copy(), b.cap.copy(), b.status.copy()


def emu_serial(b):
    L = E.lib()
    sbuf, area, ro, rl, oo, ol, st = _arrays(b)
    L.emu_zstd_decompress_batch(E._p(sbuf), C.c_uint64(len(b.stream)), E._p(ro), E._p(rl), C.c_uint32(len(b)), E._p(area),
                                E._p(oo), E._p(ol), E._p(st))
    return Result(b, area, ol, st)


def emu_par(b, **knobs):
    """min_blocks=None: the emulated gpumt_zstd_decompress_batch_par itself, at its defaults (no stats)"""
    L = E.lib()
    k = dict(KNOBS, **knobs)
    sbuf, area, ro, rl, oo, ol, st = _arrays(b)
    rp, stats = np.full(len(b), 0xA5A5A5A5, np.uint32), np.full(5, 0xA5A5A5A5, np.uint32)
    if k["min_blocks"] is None:
        assert L.gpumt_zstd_decompress_batch_par(C.c_void_p(1), E._p(sbuf), C.c_size_t(len(b.stream)), E._p(ro), E._p(rl),
                                                 C.c_size_t(len(b)), E._p(area), C.c_size_t(b.out_bytes), E._p(oo), E._p(ol),
                                                 E._p(st), E._p(rp), C.c_int(0)) == 0
        return Result(b, area, ol, st, rp, None)
    L.emu_zstd_decompress_batch_par(E._p(sbuf), C.c_uint64(len(b.stream)), E._p(ro), E._p(rl), C.c_uint32(len(b)), E._p(area),
                                    C.c_uint64(b.out_bytes), E._p(oo), E._p(ol), E._p(st), E._p(rp),
                                    C.c_uint32(k["min_blocks"]), C.c_uint32(k["slice_blocks"]), C.c_int(k["rec_par"]),
                                    C.c_uint32(k["cap_mb"]), E._p(stats))
    return Result(b, area, ol, st, rp, dict(zip(("records", "par", "blocks", "slices", "fallback"), map(int, stats))))


@contextlib.contextmanager
def captured_stderr(lines):
    """what the process writes to file descriptor 2 inside the block (the library's trace lines) -> appended to `lines`"""
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            lines += f.read().decode(errors="replace").splitlines()


def trace_stats(lines):
    """the `[gpumt zstd rec] records N par P blocks B slices S fallback F` lines -> list of dicts"""
    out = []
    for line in lines:
        if line.startswith("[gpumt zstd rec]"):
            w = line.split()
            out.append({w[i]: int(w[i + 1]) for i in range(3, 13, 2)})
    return out


class Device:
    """the two calls through an Engine that was opened with GPUMT_TRACE=1"""
    VARIANT = dict(min_blocks="zstd_rec_min_blocks", slice_blocks="zstd_rec_slice_blocks", rec_par="zstd_rec_par",
                   cap_mb="zstd_rec_cap_mb")

    def __init__(self, eng):
        self.eng = eng

    def _run(self, b, par):
        e = self.eng
        sbuf, area, ro, rl, oo, ol, st = _arrays(b)
        n = len(b)
        d_s, d_ro, d_rl, d_oo = e.upload(sbuf, slack=0), e.upload(ro), e.upload(rl), e.upload(oo)
        d_ol, d_st, d_out = e.upload(ol), e.upload(st), e.upload(area, slack=0)
        d_rp = e.upload(np.full(n, 0xA5A5A5A5, np.uint32))
        try:
            if par:
                e.zstd_decompress_par(d_s, len(b.stream), d_ro, d_rl, n, d_out, b.out_bytes, d_oo, d_ol, d_st, d_rp)
            else:
                e.zstd_decompress(d_s, len(b.stream), d_ro, d_rl, n, d_out, b.out_bytes, d_oo, d_ol, d_st)
            e.sync()
            return Result(b, e.download(d_out, len(area)), e.download(d_ol, n * 4, np.uint32),
                          e.download(d_st, n * 4, np.uint32), e.download(d_rp, n * 4, np.uint32) if par else None)
        finally:
            for d in (d_s, d_ro, d_rl, d_oo, d_ol, d_st, d_out, d_rp):
                d.free()

    def serial(self, b):
        return self._run(b, False)

    def par(self, b, **knobs):
        k = dict(KNOBS, **knobs)
        if k["min_blocks"] is None:
            del k["min_blocks"]
        prev = {name: self.eng.set_variant(self.VARIANT[name], v) for name, v in k.items()}
        assert -1 not in prev.values(), prev
        lines = []
        try:
            with captured_stderr(lines):
                r = self._run(b, True)
        finally:
            for name, v in prev.items():
                self.eng.set_variant(self.VARIANT[name], v)
        stats = trace_stats(lines)
        assert len(stats) == 1, lines
        r.stats = stats[0]
        return r


def check(b, serial, par, **knobs):
    """both calls on the same batch: status, d_out_len and bytes are the serial call's, nothing outside the records' ranges
    is written, records that came in with a status are not visited -> (serial result, par result)"""
    ref, got = serial(b), par(b, **knobs)
    assert list(got.status) == list(ref.status), (list(got.status), list(ref.status))
    assert list(got.out_len) == list(ref.out_len)
    assert ref.gaps_intact() and got.gaps_intact()
    for i, (_, cap, st_in) in enumerate(b.records):
        if st_in != 0:
            assert int(got.status[i]) == st_in and int(got.out_len[i]) == cap and int(got.rec_par[i]) == 0
            assert (np.frombuffer(got.bytes_of(i, cap), np.uint8) == CANARY).all(), i
        elif int(ref.status[i]) == 0:
            assert got.bytes_of(i, cap) == ref.bytes_of(i, cap), i        # the content and, behind it, what the capacity left
    return ref, got


# ---- records ----------------------------------------------------------------------------------------------------------------
def nblocks(fr):
    return len(Z.walk(fr)["blocks"])


def cap_of(fr, content=None, spare=100):
    """what the caller passes in d_out_len: the stated content size, else a capacity"""
    c = S.content_size_field(fr)
    if c is not None:
        return c if c <= 1 << 23 else 0
    return (len(content) if content is not None else 4096) + spare


COMMITTED = sorted(f[:-7] for f in os.listdir(GOLDEN_MT) if f.endswith(".zstdmt"))


@functools.lru_cache(maxsize=None)
def committed(name):
    """-> [frame] of every record of tests/golden/zstd/<name>.zstdmt"""
    with open(os.path.join(GOLDEN_MT, name + ".zstdmt"), "rb") as f:
        s = f.read()
    ro, rl = E.walk_records(s)
    return [s[int(o) + 12:int(o) + int(n)] for o, n in zip(ro, rl)]


def hand_frame(name, **kw):
    """a hand-built frame of zstd_par.hand_blocks() with other frame parameters"""
    kw.setdefault("window", R.WINDOW)
    kw.setdefault("fcs", 4)
    return S.frame(R.hand_blocks()[name], **kw)


def one_block_frame(n, seed):
    return S.frame([("raw", R._rnd(n, seed))], window=R.WINDOW, fcs=4)


def mixed_batch():
    """every hand-built frame, interleaved with one-block records, an empty frame and two records that come in with a
    status -> (Batch, names)"""
    recs, names = [], []
    for k, name in enumerate(R.HAND_NAMES):
        fr, want, _ = R.hand(name)
        recs.append((S.record(fr), cap_of(fr), 0))
        names.append(name)
        if k % 3 == 0:
            fr = one_block_frame(200 + k, 50 + k)
            recs.append((S.record(fr), cap_of(fr), 0))
            names.append("one_block")
        if k == 2:
            fr = S.frame([("raw", b"")], window=R.WINDOW, fcs=4)
            recs.append((S.record(fr), 0, 0))
            names.append("empty")
        if k in (4, 7):
            fr = R.hand("back_1_2_3")[0]
            recs.append((S.record(fr), cap_of(fr), 3 if k == 4 else 7))
            names.append("preset")
    return Batch(recs), names


EDGE_FRAME = "copied_thrice"      # three blocks: Raw, Compressed, Compressed


def edge_records():
    """name -> (record, capacity): what is wrong around the blocks of a 3-block frame"""
    fr, want, info = R.hand(EDGE_FRAME)
    assert len(info["blocks"]) == 3
    n = len(want)
    c = {}
    c["bytes_behind_frame"] = (S.record(fr + b"\0\0"), n)
    c["cut_in_last_block"] = (S.record(fr[:-5]), n)
    at = info["end"] - len(info["blocks"][-1]["raw"])
    bh = int.from_bytes(fr[at:at + 3], "little") + (8 << 3)
    c["last_block_claims_more"] = (S.record(fr[:at] + bh.to_bytes(3, "little") + fr[at + 3:]), n)
    c["no_last_block"] = (S.record(hand_frame(EDGE_FRAME, last=False)), n)
    c["fcs_plus_1"] = (S.record(hand_frame(EDGE_FRAME, content_size=n + 1)), n + 1)
    c["fcs_minus_1"] = (S.record(hand_frame(EDGE_FRAME, content_size=n - 1)), n - 1)
    c["dictionary_id"] = (S.record(hand_frame(EDGE_FRAME, did=5, did_width=1)), n)
    c["reserved_bit"] = (S.record(hand_frame(EDGE_FRAME, reserved=1)), n)
    c["capacity_one_short"] = (S.record(hand_frame(EDGE_FRAME, fcs=0)), n - 1)
    return c


@functools.lru_cache(maxsize=None)
def damage_record():
    """the first two blocks of the tiled stream as a frame of their own without a content size -> (frame, offset of the
    first block, bytes of the two blocks, capacity)"""
    info = P.frame(R.DAMAGE_FRAME)[2]
    blocks = [("cooked", b["raw"]) for b in info["blocks"][:R.DAMAGE_BLOCKS]]
    fr = Z.frame_of(blocks)
    total = sum(len(b["raw"]) for b in info["blocks"][:R.DAMAGE_BLOCKS])
    assert len(fr) == 6 + total
    return fr, 6, total, R.DAMAGE_BLOCKS * 131072


def damaged_batch(part, per=64):
    fr, at, total, cap = damage_record()
    recs = []
    for pos, bit in R.damage_positions(total)[per * part:per * part + per]:
        d = bytearray(fr)
        d[at + pos] ^= bit
        recs.append((S.record(bytes(d)), cap, 0))
    return Batch(recs)


def slice_batch():
    """7 hand-built records that all decode"""
    names = [n for n in R.HAND_NAMES if R.hand(n)[1] is not None][:7]
    assert len(names) == 7
    return Batch([(S.record(R.hand(n)[0]), cap_of(R.hand(n)[0]), 0) for n in names]), names


def many_blocks_batch(nrec=70, nblk=1000):
    """records of `nblk` empty Raw blocks each: 70 000 blocks, whose table alone is more than 1 MiB"""
    fr = S.frame([("raw", b"")] * nblk, window=R.WINDOW, fcs=4)
    return Batch([(S.record(fr), 0, 0)] * nrec)


def dump_cases(path):
    """the inputs of tools/zstd_rec_san.sh: the mixed batch (whole and in slices of 2 blocks), the edge cases and the damaged
    streams -> number of cases"""
    out = []

    def add(b, min_blocks=1, slice_blocks=4096):
        out.append(struct.pack("<5I", len(b.stream), len(b), b.out_bytes, min_blocks, slice_blocks) + b.stream +
                   b.rec_off.tobytes() + b.rec_len.tobytes() + b.out_off.tobytes() + b.cap.tobytes() + b.status.tobytes())
    add(mixed_batch()[0])
    add(mixed_batch()[0], slice_blocks=2)
    add(Batch([(r, c, 0) for r, c in edge_records().values()]))
    for part in range(4):
        add(damaged_batch(part))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(out))
    return len(out)
