"""Helpers of the span-index tests (TEST CODE ONLY): brotli-mt records with the index of
gpumt_brotli_compress_batch_index, batches of them through gpumt_brotli_decompress_batch_par and through
gpumt_brotli_decompress_batch on the emulator and on the device, and what tests/test_emu_brotli_rec_par.py and
tests/test_gpu_brotli_rec_par.py share.  A payload is the raw brotli stream of a record, behind its 16-byte header."""
import contextlib
import ctypes as C
import functools
import json
import os
import struct
import tempfile

import numpy as np

import emu_driver as E
import helpers as H
from golden import cases

K = 1024
BLOCK = 128 * K
MAGIC = 0x58495242                                                  # "BRIX"
CANARY = 0xCC
GAP = 7            # canary bytes between two records' output areas (odd: the areas start at every alignment)
JUNK = b"\xEE" * 3  # bytes between two records of the stream, which belong to no record
ST_OK, ST_BAD_BLOCK, ST_SIZE_MISMATCH = 0, 3, 4
QUALITIES = (1, 5, 9)                                               # one per table tier
KNOBS = dict(min_spans=2, cap=0, rec_par=1)
FOREIGN_DIR = os.path.join(H.GOLDEN_DIR, "brotli_rec")


# ---- the index --------------------------------------------------------------------------------------------------------------
def index_block(entries, n=None, magic=MAGIC):
    """the metadata meta-block of include/gpumt.h for entries [(comp_bytes, out_bytes)]"""
    body = b"".join(struct.pack("<II", c, o) for c, o in entries) + struct.pack("<II", len(entries) if n is None else n, magic)
    nb = 1 if len(body) - 1 < 256 else 2 if len(body) - 1 < 65536 else 3
    return (0x06 | nb << 4 | (len(body) - 1) << 6).to_bytes(nb + 1, "little") + body


def index_bytes(n):
    return len(index_block([(1, 1)] * n))


def with_index(payload, entries, **kw):
    """payload (ending in the empty last meta-block, 0x03) with an index for `entries` in front of that byte"""
    assert payload[-1] == 0x03
    return payload[:-1] + index_block(entries, **kw) + b"\x03"


def split_index(payload):
    """-> (the payload without its index, entries) -- (payload, None) when it has none.  Found from the end, as the
    decoder finds it; everything here is asserted, a test that damages the index builds it with index_block"""
    if len(payload) < 10 or payload[-1] != 0x03 or struct.unpack_from("<I", payload, len(payload) - 5)[0] != MAGIC:
        return payload, None
    n = struct.unpack_from("<I", payload, len(payload) - 9)[0]
    at = len(payload) - 1 - index_bytes(n)
    entries = [struct.unpack_from("<II", payload, len(payload) - 9 - 8 * (n - k)) for k in range(n)]
    assert payload[at:-1] == index_block(entries) and sum(c for c, _ in entries) == at
    return payload[:at] + b"\x03", entries


def payload_of(record):
    magic, eight, csize, br, hint = struct.unpack_from("<IIIHH", record, 0)
    assert magic == 0x184D2A50 and eight == 8 and br == 0x5242 and csize == len(record) - 16
    return record[16:], hint << 16


def records_of(stream):
    ro, rl, _ = E.walk_brotli_records(stream)
    return [stream[int(o) - 16:int(o) + int(n)] for o, n in zip(ro, rl)]


# ---- batches ----------------------------------------------------------------------------------------------------------------
class Batch:
    """records = [(payload, capacity of its output area)]"""

    def __init__(self, records):
        self.records = [(bytes(p), int(c)) for p, c in records]
        n = len(self.records)
        self.rec_off, self.rec_len = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self.out_off, self.cap = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        stream, at = bytearray(JUNK), GAP
        for i, (p, c) in enumerate(self.records):
            self.rec_off[i], self.rec_len[i] = len(stream), len(p)
            stream += p + JUNK
            self.out_off[i], self.cap[i] = at, c
            at += c + GAP
        self.stream, self.out_bytes = bytes(stream), at

    def __len__(self):
        return len(self.records)


class Result:
    def __init__(self, batch, area, out_len, status, rec_par=None, stats=None):
        self.batch, self.area, self.out_len, self.status = batch, area, out_len, status
        self.rec_par, self.stats = rec_par, stats

    def bytes_of(self, i):
        o = int(self.batch.out_off[i])
        return self.area[o:o + int(self.out_len[i])].tobytes()

    def gaps_intact(self):
        """every byte outside the records' [out_off, out_off + cap) still holds the canary"""
        keep = np.ones(len(self.area), bool)
        for o, c in zip(self.batch.out_off, self.batch.cap):
            keep[int(o):int(o) + int(c)] = False
        return bool((self.area[keep] == CANARY).all())


def _arrays(b):
    sbuf = np.frombuffer(b.stream + b"\xEE" * 320, np.uint8).copy()       # the device contract: 256 readable bytes behind
    area = np.full(b.out_bytes + 64, CANARY, np.uint8)
    return (sbuf, area, b.rec_off.copy(), b.rec_len.copy(), b.out_off.copy(), b.cap.copy(),
            np.full(len(b), 0xFFFFFFFF, np.uint32), np.full(len(b), 99, np.uint32))


@functools.lru_cache(maxsize=None)
def _blob():
    return np.frombuffer(H.brotli_blob(), np.uint8).copy()


def emu_serial(b):
    L = E.lib()
    sbuf, area, ro, rl, oo, cap, ol, st = _arrays(b)
    L.emu_brotli_decompress_batch(E._p(sbuf), E._p(ro), E._p(rl), C.c_uint32(len(b)), E._p(area), E._p(oo), E._p(cap), E._p(ol),
                                  E._p(st), E._p(_blob()), C.c_uint32(2))
    return Result(b, area, ol, st)


STAT_NAMES = ("par", "spans", "kept", "fallback")


def emu_par(b, slice_spans=1 << 20, **knobs):
    """cap: bytes of scratch the emulated device grants (0 = any)"""
    L = E.lib()
    k = dict(KNOBS, **knobs)
    if not k["rec_par"]:                                             # the switch lives in gpumt.hip: off is the serial call
        r = emu_serial(b)
        r.rec_par, r.stats = np.zeros(len(b), np.uint32), dict(records=len(b), par=0, spans=0, kept=0, fallback=0)
        return r
    sbuf, area, ro, rl, oo, cap, ol, st = _arrays(b)
    rp, info = np.full(len(b), 0xA5A5A5A5, np.uint32), np.zeros(4, np.uint64)
    L.emu_brotli_decompress_batch_par(E._p(sbuf), E._p(ro), E._p(rl), C.c_uint32(len(b)), E._p(area), E._p(oo), E._p(cap),
                                      E._p(ol), E._p(st), E._p(rp), E._p(_blob()), C.c_uint32(2), C.c_uint32(k["min_spans"]),
                                      C.c_uint64(k["cap"]), C.c_uint32(slice_spans), E._p(info))
    return Result(b, area, ol, st, rp, dict(zip(STAT_NAMES, map(int, info)), records=len(b)))


def emu_encode(data, chunk, level, index=True, win=False, grid=3):
    """-> the records (16-byte header + payload) of the emulated encoder calls"""
    L = E.lib()
    L.emu_zstd_slot_stride.restype = C.c_size_t
    L.emu_zstd_slot_stride.argtypes = [C.c_size_t]
    n = len(data)
    nrec = max(1, (n + chunk - 1) // chunk)
    stride = L.emu_zstd_slot_stride(chunk)
    inp = np.frombuffer(data + b"\xEE" * 64, np.uint8).copy()
    slots = np.full(nrec * stride, 0xEE, np.uint8)
    rec_len = np.zeros(nrec, np.uint32)
    args = (E._p(inp), C.c_uint64(n), C.c_uint32(chunk), E._p(slots), C.c_uint64(stride), E._p(rec_len), C.c_uint32(grid),
            C.c_int(level))
    if win:
        L.emu_brotli_compress_batch_win.restype = C.c_uint32
        assert L.emu_brotli_compress_batch_win(*args, C.c_uint32(0), C.c_uint64(0)) > 0
    elif index:
        L.emu_brotli_compress_batch_index(*args)
    else:
        L.emu_brotli_compress_batch_level(*args)
    assert (rec_len <= stride).all()
    return [slots[i * stride:i * stride + int(rec_len[i])].tobytes() for i in range(nrec)]


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
    """the `[gpumt brotli rec] records N par P spans S kept K fallback F` lines -> list of dicts"""
    out = []
    for line in lines:
        if line.startswith("[gpumt brotli rec]"):
            w = line.split()
            assert [w[i] for i in range(3, 13, 2)] == ["records", "par", "spans", "kept", "fallback"] and len(w) == 13, line
            out.append({w[i]: int(w[i + 1]) for i in range(3, 13, 2)})
    return out


class Device:
    """the calls through an Engine that was opened with GPUMT_TRACE=1"""
    VARIANT = dict(min_spans="brotli_rec_min_spans", cap="brotli_rec_cap_mb", rec_par="brotli_rec_par")

    def __init__(self, eng):
        self.eng = eng

    def _run(self, b, par):
        e = self.eng
        sbuf, area, ro, rl, oo, cap, ol, st = _arrays(b)
        n = len(b)
        d_s, d_ro, d_rl, d_oo, d_cap = e.upload(sbuf, slack=0), e.upload(ro), e.upload(rl), e.upload(oo), e.upload(cap)
        d_ol, d_st, d_out = e.upload(ol), e.upload(st), e.upload(area, slack=0)
        d_rp = e.upload(np.full(n, 0xA5A5A5A5, np.uint32))
        try:
            if par:
                e.brotli_decompress_par(d_s, d_ro, d_rl, n, d_out, d_oo, d_cap, d_ol, d_st, d_rp)
            else:
                e.brotli_decompress(d_s, d_ro, d_rl, n, d_out, d_oo, d_cap, d_ol, d_st)
            e.sync()
            return Result(b, e.download(d_out, len(area)), e.download(d_ol, n * 4, np.uint32),
                          e.download(d_st, n * 4, np.uint32), e.download(d_rp, n * 4, np.uint32) if par else None)
        finally:
            for d in (d_s, d_ro, d_rl, d_oo, d_cap, d_ol, d_st, d_out, d_rp):
                d.free()

    def serial(self, b):
        return self._run(b, False)

    def par(self, b, **knobs):
        """cap: MiB of scratch above which the call's own request counts as refused (0 = none)"""
        k = dict(KNOBS, **knobs)
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

    def encode(self, data, chunk, level, index=True, win=False):
        return records_of(self.eng.compress_bytes(data, chunk, codec="brotli", level=level, index=index and not win, win=win)[0])


def check(b, serial, par, **knobs):
    """both calls on the same batch: status and d_out_len are the serial call's, so are the bytes of every record that
    decoded, and nothing outside the records' output areas is written -> (serial result, par result)"""
    ref, got = serial(b), par(b, **knobs)
    print("check:", got.stats, "rec_par", list(got.rec_par[:8]), "status", list(got.status[:8]), list(ref.status[:8]),
          "out_len", list(got.out_len[:8]), list(ref.out_len[:8]))
    assert list(got.status) == list(ref.status), (list(got.status), list(ref.status))
    assert list(got.out_len) == list(ref.out_len), (list(got.out_len), list(ref.out_len))
    for i in range(len(b)):
        if int(ref.status[i]) == 0:
            assert got.bytes_of(i) == ref.bytes_of(i), i
    assert ref.gaps_intact() and got.gaps_intact()
    assert all(int(p) in (0, 1) for p in got.rec_par)
    assert all(int(s) == 0 for s, p in zip(got.status, got.rec_par) if p)
    st = got.stats
    assert st["records"] == len(b) and st["kept"] == int(sum(got.rec_par)) and st["kept"] <= st["par"] <= len(b)
    return ref, got


# ---- inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kinds():
    """name -> data of 640 KiB (five blocks, so the four groups of a wave wrap)"""
    t, r = cases.text(BLOCK, 31), cases.rnd(BLOCK, 32)
    return {"text": cases.text(5 * BLOCK, 33), "zeros": bytes(5 * BLOCK), "random": cases.rnd(5 * BLOCK, 34),
            "alternating": t + r + bytes(BLOCK) + r[::-1] + t[:BLOCK - 9]}


def light(n, seed):
    """n bytes that cost the emulator little: per 128 KiB block 2000 bytes of text, then a 300-byte period (a few long
    copies), a different one in every block"""
    out = b""
    for b in range(-(-n // BLOCK)):
        out += (cases.text(2000, seed + b) + cases.rep(cases.text(300, seed + 100 + b), BLOCK - 2000))[:BLOCK]
    return out[:n]


SIZES = {"128k+1": BLOCK + 1, "256k": 2 * BLOCK, "640k": 5 * BLOCK, "1m+77": (1 << 20) + 77}


def other_decoders(record, data):
    """the checker, libbrotli and the reference build (where they travelled) read an indexed record as any other"""
    payload, cap = payload_of(record)
    assert H.oracle_brotlimt_decompress(record, len(data) + 64) == data
    assert H.oracle_brotli_decompress(payload, len(data) + 64) == data
    if H.have_libbrotli():
        assert H.libbrotli_decompress(payload, cap) == data
    if H.have_bref():
        rv, out, _, _ = H.brotlimt_decompress_via(H.bref(), record, threads=2)
        assert rv == 0 and out == data


@functools.lru_cache(maxsize=None)
def foreign():
    """name -> (stream without index, spans, data, manifest entry) of tests/golden/brotli_rec"""
    with open(os.path.join(FOREIGN_DIR, "manifest.json")) as f:
        man = json.load(f)
    out = {}
    for name, m in sorted(man.items()):
        with open(os.path.join(FOREIGN_DIR, name + ".br"), "rb") as f:
            st = f.read()
        data = cases.text(m["bytes"], m["seed"])
        assert H.sha256(data) == m["sha256"] and len(st) == m["stream_bytes"] and st[-1] == 0x03
        out[name] = (st, [tuple(s) for s in m["spans"]], data, m)
    return out


def flip(payload, at, bit=0):
    p = bytearray(payload)
    p[at] ^= 1 << bit
    return bytes(p)


def tampered(payload):
    """name -> damaged payload, from an indexed payload of at least three spans"""
    plain, e = split_index(payload)
    assert e is not None and len(e) >= 3
    idx = len(payload) - 1 - index_bytes(len(e))                     # where the index block starts
    mod = lambda k, dc, do: e[:k] + [(e[k][0] + dc, e[k][1] + do)] + e[k + 1:]  # noqa: E731
    t = {}
    t["comp+1"], t["comp-1"] = with_index(plain, mod(1, 1, 0)), with_index(plain, mod(1, -1, 0))
    t["comp_shifted"] = with_index(plain, mod(0, 1, 0)[:1] + mod(1, -1, 0)[1:])        # the sum holds, the cut does not
    t["out+1"], t["out-1"] = with_index(plain, mod(1, 0, 1)), with_index(plain, mod(1, 0, -1))
    t["out_shifted"] = with_index(plain, mod(0, 0, 1)[:1] + mod(1, 0, -1)[1:])
    t["n+1"], t["n-1"] = with_index(plain, e, n=len(e) + 1), with_index(plain, e, n=len(e) - 1)
    t["entry_dropped"], t["entry_added"] = with_index(plain, e[:-1]), with_index(plain, e + [(1, 1)])
    t["magic"] = with_index(plain, e, magic=MAGIC ^ 0x100)
    t["comp_past_record"] = with_index(plain, mod(len(e) - 1, len(payload), 0))
    t["comp_huge"] = with_index(plain, e[:1] + [(0xFFFFFF00, e[1][1])] + e[2:])
    t["truncated"] = payload[:-20]
    t["truncated_in_span"] = payload[:e[0][0] + 10]
    t["bit_in_span_1"] = flip(payload, e[0][0] + e[1][0] // 2, 3)
    t["bit_in_span_1_header"] = flip(payload, e[0][0], 0)            # ISLAST of span 1's meta-block
    t["bit_in_index_header"] = flip(payload, idx, 4)
    t["last_byte"] = payload[:-1] + b"\x07"
    t["swapped"] = with_index(plain, [e[1], e[0]] + e[2:])
    t["zero_comp"] = with_index(plain, [(e[0][0] + e[1][0], e[0][1])] + [(0, e[1][1])] + e[2:])
    t["zero_out"] = with_index(plain, [(e[0][0], e[0][1] + e[1][1])] + [(e[1][0], 0)] + e[2:])
    return t


def dump_cases(path, encode):
    """inputs for tests/emu/brotli_rec_san.cpp: a count, then per case the payload count and per payload (bytes, capacity)
    and the bytes.  Own indexed records, the foreign ones with their index, and the tampered ones next to intact ones"""
    own = [payload_of(r) for q in QUALITIES for r in encode(light(5 * BLOCK, 80 + q), 1 << 20, q)]
    alt = [payload_of(r) for r in encode(kinds()["alternating"], 1 << 20, 1)]
    frn = [(with_index(st, spans), len(data)) for st, spans, data, _ in foreign().values()]
    good = own[0]
    todo = [own, alt, frn] + [[good, (p, good[1]), good] for _, p in sorted(tampered(good[0]).items())]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(todo)))
        for batch in todo:
            f.write(struct.pack("<I", len(batch)))
            for p, c in batch:
                f.write(struct.pack("<II", len(p), c) + p)
    return len(todo)
