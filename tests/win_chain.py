"""Helpers of the segment-parallel chain build tests (TEST CODE ONLY): the smallest inputs at which stitching the segments'
chains can go wrong, the plane through emu_win_chain_par, and the records of both window encoders with GPUMT_WIN_CHAIN_PAR
set -- under the emulator, where the variable stands in for gpumt_set_variant's "win_chain_par"."""
import ctypes as C
import os
import struct

import numpy as np

import emu_driver as E
import zstd_win as ZW
from golden import cases
from zstd_win import FAR, emu_plane, model_plane  # noqa: F401  (what the suites compare with)

K = 1024
SEG_LOG = 12                                                      # 4 KiB segments: what the shapes below are cut for


def shapes():
    """name -> (data, chunk): at seg_log 12"""
    out = {}
    for n in (4096, 4097, 4096 + 5, 4096 + 6, 8192):              # the 5 hashless positions in, across and beyond segment 1
        out["one_chunk_%d" % n] = (cases.text(n, 70 + n % 7), 1 << 20)
    out["zeros_300k"] = (bytes(300 * K), 1 << 20)                 # one chain: a segment's first position links to the last one's last
    out["period_65537"] = (cases.rep(cases.rnd(65537, 5), 300 * K), 1 << 20)  # a predecessor 16 segments back
    out["rnd_40k"] = (cases.rnd(40 * K, 81), 1 << 20)             # hashes without a predecessor stay NONE after the patch
    out["chunk_200000"] = (cases.text(600000, 13), 200000)        # segments do not divide the chunk (a last segment of 3392 = 53 * 64)
    out["chunk_100003"] = (cases.text(250000, 14), 100003)        # ... and a last segment that is no multiple of 64 (1699, 842)
    out["short_last_chunk"] = (cases.text(2 * 65536 + 5000, 82), 65536)  # the last chunk's hlog (12) is below the stride's (13)
    out["empty"] = (b"", 1 << 20)
    for n in (1, 6, 7):
        out["bytes_%d" % n] = (cases.text(n, 3), 1 << 20)
    return out


def shared_shapes(limit=300 * K):
    """the shapes above and those of zstd_win.shapes() up to `limit` bytes (the first win where a name is in both)"""
    out = {"zw_" + k: v for k, v in ZW.shapes().items() if len(v[0]) <= limit}
    out.update(shapes())
    return out


def _lib():
    L = ZW._lib()
    L.emu_win_chain_par_scratch.restype = C.c_uint64
    return L


def emu_plane_par(data, chunk, seg_log=SEG_LOG, grid=3):
    """the plane through the three launches, with a guard word behind it"""
    L = _lib()
    inp = np.frombuffer(data + b"\xEE" * 64, np.uint8).copy()
    plane = np.full(len(data) + 1, 0xA5A5A5A5, np.uint32)
    L.emu_win_chain_par(E._p(inp), C.c_uint64(len(data)), C.c_uint32(chunk), E._p(plane), C.c_uint32(seg_log), C.c_uint32(grid))
    assert int(plane[len(data)]) == 0xA5A5A5A5
    return plane[:len(data)]


def par_scratch(n, chunk, seg_log):
    return int(_lib().emu_win_chain_par_scratch(C.c_uint64(n), C.c_uint32(chunk), C.c_uint32(seg_log)))


def emu_gpumt_records(codec, data, chunk, level, par=None, cap=None):
    """the emulated gpumt_{zstd,brotli}_compress_batch_win with GPUMT_WIN_CHAIN_PAR = par and GPUMT_WIN_CHAIN_CAP = cap
    (None = unset) and GPUMT_TRACE=1 -> records; the caller reads the trace lines from stderr (capfd)"""
    L = _lib()
    L.emu_zstd_slot_stride.restype = C.c_size_t
    L.emu_zstd_slot_stride.argtypes = [C.c_size_t]
    n = len(data)
    nrec = max(1, (n + chunk - 1) // chunk)
    stride = L.emu_zstd_slot_stride(chunk)
    inp = np.frombuffer(data + b"\xEE" * 64, np.uint8).copy()
    slots = np.full(nrec * stride, 0xEE, np.uint8)
    rec_len = np.zeros(nrec, np.uint32)
    keys = {"GPUMT_WIN_CHAIN_PAR": par, "GPUMT_WIN_CHAIN_CAP": cap, "GPUMT_TRACE": "1",
            "GPUMT_ZSTD_WIN_DEPTH": None, "GPUMT_ZSTD_WIN_CAP": None, "GPUMT_BROTLI_WIN_DEPTH": None, "GPUMT_BROTLI_WIN_CAP": None}
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k, v in keys.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        call = getattr(L, "gpumt_%s_compress_batch_win" % codec)
        rv = call(C.c_void_p(1), E._p(inp), C.c_size_t(n), C.c_size_t(chunk), E._p(slots), C.c_size_t(stride), E._p(rec_len),
                  C.c_int(level), C.c_int(0))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert rv == 0
    return [slots[i * stride:i * stride + int(rec_len[i])].tobytes() for i in range(nrec)]


def chain_lines(err):
    """the [gpumt win chain] lines of a captured stderr -> dicts"""
    out = []
    for line in err.splitlines():
        if line.startswith("[gpumt win chain]"):
            w = line.split()
            out.append(dict(segments=int(w[4]), seg_log=int(w[6]), heads=int(w[8]), serial=int(w[10])))
    return out


def dump_cases(path):
    """inputs for tests/emu/win_chain_par_san.cpp: a count, then per case (bytes, chunk) and the data"""
    todo = [v for _, v in sorted(shapes().items())]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(todo)))
        for d, c in todo:
            f.write(struct.pack("<2I", len(d), c) + d)
    return len(todo)
