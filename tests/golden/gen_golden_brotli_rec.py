#!/usr/bin/env python3
"""Fixtures of the span-index decode tests (tests/brotli_rec.py): foreign brotli streams whose spans are byte-aligned but
not self-contained.  libbrotlienc 1.0.9 through ctypes: BrotliEncoderCompressStream with BROTLI_OPERATION_FLUSH after every
20 KiB of text (the last piece included), then BROTLI_OPERATION_FINISH without input -- which writes the empty last
meta-block, the single byte 0x03 that the index helper of the tests looks for.  A flush ends the meta-block and pads to a
byte boundary with an empty metadata meta-block, so every piece is a byte range of the stream; at quality 5 its matches and
its distance codes reach back into the earlier pieces.

Writes tests/golden/brotli_rec/<name>.br (the raw stream, no index) and manifest.json: per fixture the input's generator
arguments, its sha256, and the spans [[comp_bytes, out_bytes], ...].  `kept` -- whether gpumt_brotli_decompress_batch_par
keeps the record once the tests put an index in -- is recorded by hand from a run of the tests (they assert only equality
with the serial call).

Run from the repository root:  python tests/golden/gen_golden_brotli_rec.py
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402

LIB = "/opt/conda/lib/libbrotlienc.so.1"
OUT = os.path.join(HERE, "brotli_rec")
PIECE = 20 * 1024
PROCESS, FLUSH, FINISH = 0, 1, 2
MODE, QUALITY, LGWIN = 0, 1, 2

# name -> (text bytes, text seed, quality, lgwin)
FIXTURES = {
    "flush_q5_60k": (60 * 1024, 71, 5, 18),
    "flush_q5_100k_tail": (100 * 1024 + 333, 72, 5, 22),
    "flush_q1_80k": (80 * 1024, 73, 1, 18),
}
# recorded from tests/test_emu_brotli_rec_par.py::test_foreign_streams (see the docstring)
KEPT = {"flush_q5_60k": False, "flush_q5_100k_tail": False, "flush_q1_80k": True}


def encoder():
    L = C.CDLL(LIB)
    L.BrotliEncoderCreateInstance.restype = C.c_void_p
    L.BrotliEncoderCreateInstance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.BrotliEncoderSetParameter.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.BrotliEncoderCompressStream.restype = C.c_int
    L.BrotliEncoderCompressStream.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.BrotliEncoderHasMoreOutput.argtypes = [C.c_void_p]
    L.BrotliEncoderDestroyInstance.argtypes = [C.c_void_p]
    return L


def flushed(data, quality, lgwin):
    """-> (stream, [(comp_bytes, out_bytes)])"""
    L = encoder()
    st = L.BrotliEncoderCreateInstance(None, None, None)
    assert st
    assert L.BrotliEncoderSetParameter(st, QUALITY, quality) and L.BrotliEncoderSetParameter(st, LGWIN, lgwin)
    assert L.BrotliEncoderSetParameter(st, MODE, 0)
    src = C.create_string_buffer(data, len(data))
    cap = len(data) + 4096
    dst = C.create_string_buffer(cap)
    stream, spans = b"", []

    def step(op, at, n):
        avail_in, next_in = C.c_size_t(n), C.c_void_p(C.addressof(src) + at)
        got = b""
        while True:
            avail_out, next_out = C.c_size_t(cap), C.c_void_p(C.addressof(dst))
            assert L.BrotliEncoderCompressStream(st, op, C.byref(avail_in), C.byref(next_in), C.byref(avail_out),
                                                 C.byref(next_out), None) == 1
            got += dst.raw[:cap - avail_out.value]
            if avail_in.value == 0 and not L.BrotliEncoderHasMoreOutput(st):
                return got

    for at in range(0, len(data), PIECE):
        n = min(PIECE, len(data) - at)
        piece = step(FLUSH, at, n)
        stream += piece
        spans.append((len(piece), n))
    stream += step(FINISH, len(data), 0)
    L.BrotliEncoderDestroyInstance(st)
    return stream, spans


def main():
    os.makedirs(OUT, exist_ok=True)
    manifest = {}
    for name, (n, seed, quality, lgwin) in sorted(FIXTURES.items()):
        data = cases.text(n, seed)
        stream, spans = flushed(data, quality, lgwin)
        assert stream[-1] == 0x03 and sum(c for c, _ in spans) == len(stream) - 1, (name, stream[-1])
        assert sum(o for _, o in spans) == len(data) and len(stream) < 64 * 1024
        with open(os.path.join(OUT, name + ".br"), "wb") as f:
            f.write(stream)
        manifest[name] = dict(bytes=n, seed=seed, quality=quality, lgwin=lgwin, sha256=hashlib.sha256(data).hexdigest(),
                              stream_bytes=len(stream), spans=[list(s) for s in spans], kept=KEPT[name])
        print(name, len(data), "->", len(stream), "bytes,", len(spans), "spans")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
