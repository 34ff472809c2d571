"""Helpers of the whole-chunk-window brotli encoder tests (TEST CODE ONLY): gpumt_brotli_compress_batch_win under the
emulator, the shape list it shares with the zstd window tests, the inputs of the far-repeat and distance-cap cases, and the
decoders every stream goes through."""
import ctypes as C
import struct

import numpy as np

import emu_driver as E
import helpers as H
import zstd_win as ZW
from golden import cases

QUALITIES = (9, 10, 11)
K = 1024
shapes = ZW.shapes
soups = ZW.soups

FAR = cases.rnd(256 * K, 9) * 2                                   # the second copy lies 262144 behind the first: beyond 2^18 - 16
FAR_BOUND = 256 * K + 8 * K                                       # the first copy stored + the zstd test's 8 KiB margin

CAP_CHUNK = 17 << 20
CAP_NOISE = 70 * K
CAP_TAKEN, CAP_REFUSED = (1 << 24) - 16, (1 << 24) - 15          # the largest distance of WBITS 24, and one more


def cap_input(dist):
    """A + zeros + A: the second A starts `dist` behind the first, everything in one record of a 17 MiB chunk"""
    a = cases.rnd(CAP_NOISE, 3)
    return a + bytes(dist - CAP_NOISE) + a


def wbits_of(stream):
    """the WBITS a brotli-mt stream's first record declares (RFC 7932 9.1; the encoder writes 18..24: "1" + three bits)"""
    b = stream[16]
    assert b & 1
    return 17 + ((b >> 1) & 7)


# ---- the new call under the emulator -------------------------------------------------------------------------------------
def _lib():
    L = E.lib()
    L.emu_zstd_slot_stride.restype = C.c_size_t
    L.emu_zstd_slot_stride.argtypes = [C.c_size_t]
    L.emu_brotli_compress_batch_win.restype = C.c_uint32
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
        ran = L.emu_brotli_compress_batch_win(E._p(inp), C.c_uint64(n), C.c_uint32(chunk), E._p(slots), C.c_uint64(stride),
                                              E._p(rec_len), C.c_uint32(grid), C.c_int(level), C.c_uint32(depth), C.c_uint64(cap))
    else:
        ran = 0
        L.emu_brotli_compress_batch_level(E._p(inp), C.c_uint64(n), C.c_uint32(chunk), E._p(slots), C.c_uint64(stride),
                                          E._p(rec_len), C.c_uint32(grid), C.c_int(level))
    return [slots[i * stride:i * stride + int(rec_len[i])].tobytes() for i in range(nrec)], int(ran)


def emu_stream(data, chunk, level, **kw):
    return b"".join(emu_records(data, chunk, level, **kw)[0])


# ---- the decoders --------------------------------------------------------------------------------------------------------
def decode_all(stream, data, emu=True):
    """the oracle, both emulated decoder kernels (emu), libbrotli and the reference build where present"""
    assert H.oracle_brotlimt_decompress(stream, len(data) + 64) == data
    if emu:
        import os
        for variant in (None, "1"):                               # dec4 first / the general kernel alone
            old = os.environ.pop("EMU_BROTLI_DEC", None)
            if variant:
                os.environ["EMU_BROTLI_DEC"] = variant
            try:
                recs, status = E.brotli_decompress(stream)
            finally:
                os.environ.pop("EMU_BROTLI_DEC", None)
                if old is not None:
                    os.environ["EMU_BROTLI_DEC"] = old
            assert (status == 0).all() and b"".join(recs) == data, variant
    if H.have_libbrotli():
        ro, rl, cap = E.walk_brotli_records(stream)
        got = [H.libbrotli_decompress(stream[int(o):int(o) + int(n)], int(c)) for o, n, c in zip(ro, rl, cap)]
        assert None not in got and b"".join(got) == data
    if H.have_bref():
        rv, out, _, _ = H.brotlimt_decompress_via(H.bref(), stream, threads=2)
        assert rv == 0 and out == data


def dump_cases(path):
    """inputs for tests/emu/brotli_win_san.cpp: a count, then per case (bytes, chunk, quality) and the data"""
    todo = [(d, c, q) for name, (d, c) in sorted(shapes().items()) for q in (9, 11)
            if len(d) <= 300 * K and name not in ("period_65537", "dense_sequences")]
    todo.append((FAR, 1 << 20, 9))
    todo.append((cases.text(5 * 3000, 8), 3000, 11))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(todo)))
        for d, c, q in todo:
            f.write(struct.pack("<3I", len(d), c, q) + d)
    return len(todo)
