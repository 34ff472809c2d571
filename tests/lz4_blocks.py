"""Helpers of the block-level plain .lz4 tests (TEST CODE ONLY): an LZ4 frame split into the block table and run list
gpumt_lz4_decompress_blocks takes, the emulated kernel over them, and the emulated host library with small batches."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_driver as E
import helpers as H
from zstdmt_amd.device import LZ4_BLOCK, LZ4_RUN, XXH32_JOB, LZ4B_STORED, LZ4B_CHECKSUM

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
ERR = lambda e: C.c_size_t(-e).value  # noqa: E731
E_LIB = 8


def walk(fr: bytes):
    """frame -> dict(indep, bchk, cchk, csize (None if absent), blkmax, blocks [(stored, body, checksum)], expect)"""
    assert struct.unpack_from("<I", fr, 0)[0] == 0x184D2204
    flg, bd = fr[4], fr[5]
    at = 6
    csize = None
    if flg & 8:
        csize = struct.unpack_from("<Q", fr, at)[0]
        at += 8
    if flg & 1:
        at += 4
    at += 1
    info = dict(indep=bool(flg & 0x20), bchk=bool(flg & 0x10), cchk=bool(flg & 4), csize=csize,
                blkmax=1 << (8 + 2 * (bd >> 4)), blocks=[], expect=None)
    while True:
        bh = struct.unpack_from("<I", fr, at)[0]
        at += 4
        if bh == 0:
            break
        n = bh & 0x7FFFFFFF
        body = fr[at:at + n]
        assert len(body) == n
        at += n
        chk = 0
        if info["bchk"]:
            chk = struct.unpack_from("<I", fr, at)[0]
            at += 4
        info["blocks"].append((bool(bh >> 31), body, chk))
    if info["cchk"]:
        info["expect"] = struct.unpack_from("<I", fr, at)[0]
        at += 4
    info["end"] = at
    return info


def tables(info, history=0):
    """(stream bytes, LZ4_BLOCK[n], LZ4_RUN[m], out_bytes) the way the host engine lays a frame out: every block of an
    independent frame in its own slot, the blocks of a linked frame in one run behind `history` bytes"""
    blocks = np.zeros(len(info["blocks"]), LZ4_BLOCK)
    runs, stream, out = [], bytearray(), history
    for i, (stored, body, chk) in enumerate(info["blocks"]):
        blocks[i] = (len(stream), len(body), (LZ4B_STORED if stored else 0) | (LZ4B_CHECKSUM if info["bchk"] else 0),
                     info["blkmax"], chk)
        stream += body
        cap = len(body) if stored else min(info["blkmax"], 255 * len(body))
        if info["indep"] or not runs:
            runs.append([out if info["indep"] else 0, out, 0, i, 0, 0])
        runs[-1][2] += cap
        runs[-1][4] += 1
        out += cap
    r = np.zeros(len(runs), LZ4_RUN)
    for i, v in enumerate(runs):
        r[i] = tuple(v)
    return bytes(stream), blocks, r, out


def emu_decode_blocks(stream, blocks, runs, out_bytes, history=b"", pack=False):
    """emu_lz4_decompress_blocks (+ emu_lz4_pack_runs) -> (output, block_len, run_len, status)"""
    L = E.lib()
    nblk, nrun = len(blocks), len(runs)
    sbuf = np.frombuffer(bytes(stream) + b"\xEE" * 8, np.uint8).copy()
    area = np.full(out_bytes + 64, 0xCC, np.uint8)
    area[:len(history)] = np.frombuffer(history, np.uint8)
    bl, rl, st = np.zeros(nblk + 1, np.uint32), np.full(nrun, 0xA5A5A5A5, np.uint32), np.full(nrun, 99, np.uint32)
    blocks, runs = np.ascontiguousarray(blocks), np.ascontiguousarray(runs)
    L.emu_lz4_decompress_blocks(E._p(sbuf), C.c_uint64(len(stream)), E._p(blocks), C.c_uint32(nblk), E._p(runs),
                                C.c_uint32(nrun), E._p(area), C.c_uint64(out_bytes), E._p(bl), E._p(rl), E._p(st))
    assert (area[out_bytes:] == 0xCC).all(), "decoder wrote past the end of its output"
    out = area[:out_bytes].tobytes()
    if pack:
        packed = np.full(out_bytes + 64, 0xDD, np.uint8)
        po = np.zeros(nrun + 1, np.uint64)
        L.emu_lz4_pack_runs(E._p(area), C.c_uint64(out_bytes), E._p(runs), E._p(rl), C.c_uint32(nrun), E._p(packed),
                            C.c_uint64(out_bytes), E._p(po))
        assert (packed[int(po[nrun]):] == 0xDD).all()
        out = packed[:int(po[nrun])].tobytes()
    return out, bl[:nblk], rl, st


def emu_xxh32_carry(data: bytes, pieces):
    """XXH32 of data continued over `pieces` by the emulated carried-state kernel -> digest"""
    L = E.lib()
    buf = np.frombuffer(data + b"\0" * 16, np.uint8).copy()
    states = np.full(24, 0xA5A5A5A5, np.uint32)
    dig, ver = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    at, xs = 0, 0
    for i, n in enumerate(pieces):
        last = i == len(pieces) - 1
        job = np.zeros(1, XXH32_JOB)
        job["off"], job["len"] = at, n
        job["flags"] = (1 if i == 0 else xs << 8) | (2 if last else (xs ^ 1) << 9)
        if not last:
            xs ^= 1
        L.emu_xxh32_carry(E._p(buf), C.c_uint64(len(data)), E._p(job), C.c_uint32(1), E._p(states), E._p(dig), E._p(ver))
        at += n
    return int(dig[0])


_host = None


def host_lib(batch_kb=16):
    """the host engines over the emulated device, with batches of batch_kb KiB (read once by the library)"""
    global _host
    if _host is None:
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        old = os.environ.get("GPUMT_BATCH_KB")
        os.environ["GPUMT_BATCH_KB"] = str(batch_kb)
        L = H.bind_lz4mt(C.CDLL(os.path.join(EMU_DIR, "libzstdmt_emu_host.so")))
        rv, _, _, _ = H.lz4mt_compress_via(L, b"prime", 4096)     # primes the cached batch size while the variable is set
        assert rv == 0
        if old is None:
            os.environ.pop("GPUMT_BATCH_KB", None)
        else:
            os.environ["GPUMT_BATCH_KB"] = old
        _host = L
    return _host
