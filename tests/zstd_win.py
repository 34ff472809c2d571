"""Helpers of the whole-chunk-window zstd encoder tests (TEST CODE ONLY): gpumt_zstd_compress_batch_win under the emulator
and on the device, the shape list both suites share, a model of the chain plane in plain Python, and the three decoders
every stream goes through."""
import ctypes as C
import json
import random

import numpy as np

import emu_driver as E
import helpers as H
from golden import cases

LEVELS = (10, 16, 19, 22)
HBYTES, HLOG_MAX, HLOG_MIN, NONE = 6, 17, 12, 0xFFFFFFFF
K = 1024


def json_lines():
    """the structured input of test_emu_many_small_chunks_matches_end_with_their_block: repeat offsets"""
    return ("".join(json.dumps({"id": i, "name": "user%d" % (i * 7919 % 1000), "tags": ["a", "b", "c"][:i % 4],
                                "score": (i * 31) % 100 / 10, "active": i % 3 == 0}) + "\n" for i in range(9000))).encode()


def shapes():
    """name -> (data, chunk): the smallest inputs at which the window encoder can still go wrong"""
    out = {"empty": (b"", 1 << 20)}
    for n in (1, 6, 7, 8):
        out["bytes_%d" % n] = (cases.text(n, 3), 1 << 20)
    out["window_equals_block"] = (cases.text(2 * 131072 + 3000, 11), 131072)
    out["text_300k"] = (cases.text(300 * K, 12), 1 << 20)
    out["chunk_200000"] = (cases.text(600000, 13), 200000)       # chunk-relative positions, chunk no multiple of the block
    out["chunk_1024"] = (cases.text(300 * K, 33), 1024)          # never a source in the neighbour chunk
    out["zeros_300k"] = (bytes(300 * K), 1 << 20)                # every position on one chain
    out["period_300"] = (cases.rep(cases.rnd(300, 4), 300 * K), 1 << 20)
    out["period_65537"] = (cases.rep(cases.rnd(65537, 5), 300 * K), 1 << 20)
    out["mixed"] = (cases.rnd(70 * K, 6) + bytes(90 * K) + cases.text(100 * K, 7) + cases.rnd(40 * K, 6), 1 << 20)
    out["dense_sequences"] = (H.dense_sequences(200 * K), 1 << 20)
    out["json_lines"] = (json_lines(), 200000)
    return out


def soups(count=8, n=300 * K):
    out = {}
    for seed in range(count):
        rng = random.Random(9100 + seed)
        out["soup_%d" % seed] = (H.soup(rng, rng.randrange(n // 2, n)), rng.choice([1 << 20, 200000, 131072, 65536]), rng)
    return out


FAR = cases.rnd(192 * K, 9) * 2                                   # the second copy lies 192 KiB behind the first
FAR_BOUND = 204800                                                # the first copy stored + 8 KiB


# ---- the new call under the emulator -------------------------------------------------------------------------------------
def _lib():
    L = E.lib()
    L.emu_zstd_slot_stride.restype = C.c_size_t
    L.emu_zstd_slot_stride.argtypes = [C.c_size_t]
    L.emu_zstd_compress_batch_win.restype = C.c_uint32
    return L


def emu_records(data, chunk, level, grid=3, depth=0, cap=0, call="win"):
    """-> (records as a list of bytes, the depth the window encoder ran with -- 0 where the table encoder ran)"""
    L = _lib()
    n = len(data)
    nrec = max(1, (n + chunk - 1) // chunk)
    stride = L.emu_zstd_slot_stride(chunk)
    inp = np.frombuffer(data + b"\xEE" * 64, np.uint8).copy()
    slots = np.full(nrec * stride, 0xEE, np.uint8)
    rec_len = np.zeros(nrec, np.uint32)
    if call == "win":
        ran = L.emu_zstd_compress_batch_win(E._p(inp), C.c_uint64(n), C.c_uint32(chunk), E._p(slots), C.c_uint64(stride),
                                            E._p(rec_len), C.c_uint32(grid), C.c_int(level), C.c_uint32(depth), C.c_uint64(cap))
    else:
        ran = 0
        L.emu_zstd_compress_batch_level(E._p(inp), C.c_uint64(n), C.c_uint32(chunk), E._p(slots), C.c_uint64(stride),
                                        E._p(rec_len), C.c_uint32(grid), C.c_int(level))
    return [slots[i * stride:i * stride + int(rec_len[i])].tobytes() for i in range(nrec)], int(ran)


def emu_stream(data, chunk, level, **kw):
    return b"".join(emu_records(data, chunk, level, **kw)[0])


def emu_plane(data, chunk, grid=3):
    L = _lib()
    inp = np.frombuffer(data + b"\xEE" * 64, np.uint8).copy()
    plane = np.full(len(data) + 1, 0xA5A5A5A5, np.uint32)
    L.emu_zstd_win_chain(E._p(inp), C.c_uint64(len(data)), C.c_uint32(chunk), E._p(plane), C.c_uint32(grid))
    assert int(plane[len(data)]) == 0xA5A5A5A5
    return plane[:len(data)]


def model_plane(data, chunk):
    """prev[p] = the nearest earlier position of p's chunk with the same hash of HBYTES bytes, else NONE; the chunk's last
    HBYTES - 1 positions have none"""
    out = np.full(len(data), NONE, np.uint32)
    for c0 in range(0, len(data), chunk):
        part = data[c0:c0 + chunk]
        hlog = min(HLOG_MAX, max(HLOG_MIN, len(part).bit_length() - 1 - 3))
        last = {}
        for p in range(len(part) - HBYTES + 1):
            v = int.from_bytes(part[p:p + HBYTES], "little")
            h = (((v << (64 - 8 * HBYTES)) * 0x9E3779B185EBCA87) & (2 ** 64 - 1)) >> (64 - HLOG_MAX) >> (HLOG_MAX - hlog)
            if h in last:
                out[c0 + p] = last[h]
            last[h] = p
    return out


# ---- the three decoders --------------------------------------------------------------------------------------------------
def decode_all(stream, data, emu=True):
    """the oracle, the emulated decoder kernels (emu) and the reference build where present"""
    assert H.oracle_zstdmt_decompress(stream, len(data) + 64) == data
    if emu:
        out, status = E.zstd_decompress(stream)
        assert (status == 0).all() and out == data
    if H.have_zref():
        rv, out, _, _ = H.zstdmt_decompress_via(H.zref(), stream, threads=2)
        assert rv == 0 and out == data


def dump_cases(path):
    """inputs for tests/emu/zstd_win_san.cpp: a count, then per case (bytes, chunk, level) and the data"""
    import struct
    todo = [(d, c, lv) for name, (d, c) in sorted(shapes().items()) for lv in (10, 19)
            if len(d) <= 300 * K and name not in ("period_65537", "dense_sequences")]
    todo.append((FAR, 1 << 20, 10))
    todo.append((cases.text(5 * 3000, 8), 3000, 19))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(todo)))
        for d, c, lv in todo:
            f.write(struct.pack("<3I", len(d), c, lv) + d)
    return len(todo)
