"""Thin object wrapper over the gpumt_* C ABI (include/gpumt.h) for tests and bench.py.

Device buffers are plain integers (device pointers) owned by the Engine; numpy arrays are only
used to stage host data.  Every call that fails raises NativeError with the HIP error text.
"""
import ctypes as C

import numpy as np

from ._native import NativeError, lib

ST_NAMES = {0: "ok", 1: "bad_record", 2: "bad_frame", 3: "bad_block", 4: "size_mismatch",
            5: "bad_checksum", 6: "trailing", 7: "unsupported"}


# gpumt_lz4_block / gpumt_lz4_run / gpumt_xxh32_job (include/gpumt.h) as numpy record types
LZ4_BLOCK = np.dtype([("src_off", "<u8"), ("src_len", "<u4"), ("flags", "<u4"), ("blkmax", "<u4"), ("checksum", "<u4")])
LZ4_RUN = np.dtype([("low", "<u8"), ("out_off", "<u8"), ("out_cap", "<u4"), ("first", "<u4"), ("count", "<u4"),
                    ("reserved", "<u4")])
XXH32_JOB = np.dtype([("off", "<u8"), ("len", "<u4"), ("flags", "<u4"), ("expect", "<u4"), ("reserved", "<u4")])
# gpumt_zstd_block / gpumt_zstd_run
ZSTD_BLOCK = np.dtype([("src_off", "<u8"), ("src_len", "<u4"), ("block_max", "<u4")])
ZSTD_RUN = np.dtype([("out_off", "<u8"), ("out_cap", "<u4"), ("hist", "<u4"), ("first", "<u4"), ("count", "<u4"),
                     ("flags", "<u4"), ("carry", "<u4")])
ZRUN_FIRST, ZRUN_LAST = 1, 2
ZSTD_CARRY_BYTES = 9280
XXH64_STATE_WORDS = 20
LZ4B_STORED, LZ4B_CHECKSUM = 1, 2
XXH_RESET, XXH_FINAL, XXH_VERIFY = 1, 2, 4


class DevBuf:
    __slots__ = ("ptr", "nbytes", "eng")

    def __init__(self, eng, nbytes):
        self.eng = eng
        self.nbytes = int(nbytes)
        self.ptr = lib().gpumt_malloc(eng.h, self.nbytes)
        if not self.ptr:
            raise NativeError(f"gpumt_malloc({nbytes}) failed")

    def free(self):
        if self.ptr:
            lib().gpumt_device_sync(self.eng.h)   # gpumt_free wants an idle buffer (it may be cached and reused)
            lib().gpumt_free(self.eng.h, self.ptr)
            self.ptr = None

    def at(self, byte_off):
        return C.c_void_p(self.ptr + int(byte_off))


class Engine:
    """One HIP device. `Engine(0)` raises NativeError when no gfx950 GPU is usable."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.gpumt_open(device, C.byref(h))
        if rc != 0:
            raise NativeError(f"gpumt_open({device}) failed with {rc} (no gfx950 device / HIP runtime)")
        self.h = h
        self.name = self.L.gpumt_device_name(h).decode()

    def close(self):
        if self.h:
            self.L.gpumt_close(self.h)
            self.h = None

    # ---- helpers ---------------------------------------------------------------------------
    def _ck(self, rc, what):
        if rc != 0:
            raise NativeError(f"{what} -> {rc}: {self.L.gpumt_last_error(self.h).decode()}")

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def upload(self, arr, stream=0, slack=256):
        """numpy array / bytes -> new device buffer (+slack: 8-byte hash reads of the encoder and the
        128-byte line fetches of the decoder's parse kernel stay inside the allocation)"""
        a = np.frombuffer(arr, np.uint8) if isinstance(arr, (bytes, bytearray)) else arr
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes + slack)
        if a.nbytes:
            self._ck(self.L.gpumt_memcpy_h2d(self.h, d.ptr, a.ctypes.data, a.nbytes, stream), "h2d")
            self.sync(stream)
        return d

    def download(self, d, nbytes, dtype=np.uint8, offset=0, stream=0):
        out = np.empty(int(nbytes), np.uint8)
        if nbytes:
            self._ck(self.L.gpumt_memcpy_d2h(self.h, out.ctypes.data, d.ptr + int(offset), int(nbytes),
                                             stream), "d2h")
            self.sync(stream)
        return out.view(dtype)

    def equal(self, d_a, d_b, nbytes, piece=128 << 20):
        """byte-for-byte comparison of two device buffers: both are copied to pinned host memory in
        pieces and compared there (bench.py's round-trip verification)"""
        nbytes = int(nbytes)
        if nbytes == 0:
            return True
        piece = min(piece, nbytes)
        self.L.gpumt_host_alloc.restype = C.c_void_p
        ha = self.L.gpumt_host_alloc(self.h, piece)
        hb = self.L.gpumt_host_alloc(self.h, piece)
        if not ha or not hb:
            raise NativeError("gpumt_host_alloc failed")
        libc = C.CDLL(None)
        libc.memcmp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        same = True
        try:
            for off in range(0, nbytes, piece):
                m = min(piece, nbytes - off)
                self._ck(self.L.gpumt_memcpy_d2h(self.h, C.c_void_p(ha), d_a.ptr + off, m, 2), "d2h")
                self._ck(self.L.gpumt_memcpy_d2h(self.h, C.c_void_p(hb), d_b.ptr + off, m, 3), "d2h")
                self.sync(2)
                self.sync(3)
                if libc.memcmp(ha, hb, m) != 0:
                    same = False
                    break
        finally:
            self.L.gpumt_host_free(self.h, C.c_void_p(ha))
            self.L.gpumt_host_free(self.h, C.c_void_p(hb))
        return same

    def replicas_equal(self, d_buf, base_n, reps, piece=1 << 20, stream=0):
        """every one of `reps` back-to-back replicas of `base_n` bytes in d_buf equals replica 0: XXH32 of each `piece`
        on the device (gpumt_xxh32_batch, one pass at HBM speed), the hash rows compared on the host -- bench.py's check
        of the replicated decode legs beyond the first replica, which is compared with the text byte for byte"""
        base_n, reps = int(base_n), int(reps)
        if reps <= 1 or base_n == 0:
            return True
        per = (base_n + piece - 1) // piece
        off1 = np.arange(per, dtype=np.uint64) * np.uint64(piece)
        len1 = np.full(per, piece, np.uint32)
        len1[-1] = base_n - (per - 1) * piece
        off = np.concatenate([off1 + np.uint64(r * base_n) for r in range(reps)])
        d_off, d_len = self.upload(off, stream), self.upload(np.tile(len1, reps), stream)
        d_hash = self.alloc(per * reps * 4)
        try:
            self._ck(self.L.gpumt_xxh32_batch(self.h, d_buf.ptr, d_off.ptr, d_len.ptr, per * reps, d_hash.ptr, stream),
                     "xxh32_batch")
            hh = self.download(d_hash, per * reps * 4, np.uint32, stream=stream).reshape(reps, per)
        finally:
            for b in (d_off, d_len, d_hash):
                b.free()
        return bool((hh == hh[0]).all())

    def sync(self, stream=None):
        if stream is None:
            self._ck(self.L.gpumt_device_sync(self.h), "device_sync")
        else:
            self._ck(self.L.gpumt_stream_sync(self.h, stream), "stream_sync")

    def timer_start(self, slot, stream=0):
        self._ck(self.L.gpumt_timer_start(self.h, slot, stream), "timer_start")

    def timer_stop(self, slot, stream=0):
        self._ck(self.L.gpumt_timer_stop(self.h, slot, stream), "timer_stop")

    def timer_ms(self, slot):
        ms = C.c_float()
        self._ck(self.L.gpumt_timer_ms(self.h, slot, C.byref(ms)), "timer_ms")
        return ms.value

    def set_variant(self, what, v):
        return self.L.gpumt_set_variant(self.h, what.encode(), v)

    # ---- LZ4, device-resident ----------------------------------------------------------------
    def slot_stride(self, chunk):
        return self.L.gpumt_lz4_slot_stride(chunk)

    def record_count(self, n, chunk):
        return self.L.gpumt_lz4_record_count(n, chunk)

    def lz4_compress(self, d_in, n, chunk, d_slots, stride, d_rec_len, stream=0, level=1):
        self._ck(self.L.gpumt_lz4_compress_batch_level(self.h, d_in.ptr, n, chunk, d_slots.ptr, stride,
                                                       d_rec_len.ptr, level, stream),
                 "lz4_compress_batch_level")

    def lz4_compact(self, d_slots, stride, d_rec_len, nrec, d_stream, d_rec_off, stream=0):
        self._ck(self.L.gpumt_lz4_compact(self.h, d_slots.ptr, stride, d_rec_len.ptr, nrec,
                                          d_stream.ptr, d_rec_off.ptr, stream), "lz4_compact")

    def lz4_probe(self, d_stream, d_rec_off, d_rec_len, nrec, d_out_len, d_out_off, stream=0):
        self._ck(self.L.gpumt_lz4_probe_sizes(self.h, d_stream.ptr, d_rec_off.ptr, d_rec_len.ptr, nrec,
                                              d_out_len.ptr, d_out_off.ptr, stream), "lz4_probe_sizes")

    def lz4_decompress(self, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes,
                       d_out_off, d_out_len, d_status, stream=0):
        self._ck(self.L.gpumt_lz4_decompress_batch(self.h, d_stream.ptr, int(stream_bytes),
                                                   d_rec_off.ptr, d_rec_len.ptr, nrec, d_out.ptr,
                                                   int(out_bytes), d_out_off.ptr, d_out_len.ptr,
                                                   d_status.ptr, stream), "lz4_decompress_batch")

    def lz4_decompress_par(self, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes,
                           d_out_off, d_out_len, d_status, d_rec_par=None, stream=0):
        """gpumt_lz4_decompress_batch_par: lz4_decompress with the records of several linked blocks decoded block-parallel;
        d_rec_par (nrec words, may be None) receives per record the blocks that route decoded and kept"""
        self._ck(self.L.gpumt_lz4_decompress_batch_par(self.h, d_stream.ptr, int(stream_bytes), d_rec_off.ptr,
                                                       d_rec_len.ptr, nrec, d_out.ptr, int(out_bytes), d_out_off.ptr,
                                                       d_out_len.ptr, d_status.ptr,
                                                       d_rec_par.ptr if d_rec_par is not None else None, stream),
                 "lz4_decompress_batch_par")

    def lz4_decompress_par_bytes(self, stream: bytes, rec_off, rec_len):
        """decompress_bytes for lz4-mt records through lz4_decompress_par -> (content bytes, status[n], rec_par[n])"""
        nrec = len(rec_len)
        d_stream = self.upload(stream)
        d_ro = self.upload(np.asarray(rec_off, np.uint64)[:nrec].copy())
        d_rl = self.upload(np.asarray(rec_len, np.uint32).copy())
        d_ol, d_oo, d_st, d_rp = self.alloc(nrec * 4), self.alloc((nrec + 1) * 8), self.alloc(nrec * 4), self.alloc(nrec * 4)
        try:
            self.lz4_probe(d_stream, d_ro, d_rl, nrec, d_ol, d_oo)
            total = int(self.download(d_oo, (nrec + 1) * 8, np.uint64)[nrec])
            d_out = self.alloc(total + 64)
            try:
                lib().gpumt_memset(self.h, d_out.ptr, 0xCC, total + 64, 0)
                self.lz4_decompress_par(d_stream, len(stream), d_ro, d_rl, nrec, d_out, total, d_oo, d_ol, d_st, d_rp)
                status = self.download(d_st, nrec * 4, np.uint32)
                rec_par = self.download(d_rp, nrec * 4, np.uint32)
                raw = self.download(d_out, total + 64)
                assert (raw[total:] == 0xCC).all(), "decoder wrote past the end of its output"
            finally:
                d_out.free()
        finally:
            for b in (d_stream, d_ro, d_rl, d_ol, d_oo, d_st, d_rp):
                b.free()
        return raw[:total].tobytes(), status, rec_par

    def lz4_decompress_blocks(self, stream: bytes, blocks, runs, out_bytes, history=b"", pack=False, blk_fill=0,
                              call="gpumt_lz4_decompress_blocks"):
        """gpumt_lz4_decompress_blocks over host bytes: `blocks` / `runs` are LZ4_BLOCK / LZ4_RUN arrays, `history` is
        placed at the start of the output (what a linked run reads behind its `low`).  -> (output area bytes,
        block_len[nblk], run_len[nrun], status[nrun]); with pack=True the output is what gpumt_lz4_pack_runs made of
        the runs, in order.  block_len starts as `blk_fill`: the words of blocks that were not decoded keep it."""
        blocks = np.ascontiguousarray(blocks, LZ4_BLOCK)
        runs = np.ascontiguousarray(runs, LZ4_RUN)
        nblk, nrun = len(blocks), len(runs)
        area = np.full(int(out_bytes) + 64, 0xCC, np.uint8)
        area[:len(history)] = np.frombuffer(history, np.uint8)
        d_stream = self.upload(stream, slack=0) if stream else self.alloc(64)
        d_blk, d_run, d_out = self.upload(blocks.view(np.uint8)), self.upload(runs.view(np.uint8)), self.upload(area, slack=0)
        d_bl = self.upload(np.full(nblk + 1, blk_fill, np.uint32))
        d_rl, d_st = self.alloc(nrun * 4), self.alloc(nrun * 4)
        d_pk, d_po = self.alloc(int(out_bytes) + 64), self.alloc((nrun + 1) * 8)
        seg = call == "gpumt_lz4_decompress_blocks_seg"
        d_bs = self.upload(np.full(nblk + 1, 0xA5A5A5A5, np.uint32)) if seg else None
        try:
            self._ck(getattr(self.L, call)(self.h, d_stream.ptr, len(stream), d_blk.ptr, nblk, d_run.ptr, nrun,
                                           d_out.ptr, int(out_bytes), d_bl.ptr, d_rl.ptr, d_st.ptr,
                                           *((d_bs.ptr, 0) if seg else (0,))), call[6:])
            status = self.download(d_st, nrun * 4, np.uint32)
            run_len = self.download(d_rl, nrun * 4, np.uint32)
            blk_len = self.download(d_bl, nblk * 4, np.uint32)
            raw = self.download(d_out, int(out_bytes) + 64)
            assert (raw[int(out_bytes):] == 0xCC).all(), "decoder wrote past the end of its output"
            out = raw[:int(out_bytes)].tobytes()
            if pack:
                self._ck(self.L.gpumt_lz4_pack_runs(self.h, d_out.ptr, int(out_bytes), d_run.ptr, d_rl.ptr, nrun, d_pk.ptr,
                                                    int(out_bytes), d_po.ptr, 0), "lz4_pack_runs")
                total = int(self.download(d_po, (nrun + 1) * 8, np.uint64)[nrun])
                out = self.download(d_pk, total).tobytes()
            if seg:
                blk_seg = self.download(d_bs, (nblk + 1) * 4, np.uint32)
                assert int(blk_seg[nblk]) == 0xA5A5A5A5, "decoder wrote past the end of block_seg"
                return out, blk_len, run_len, status, blk_seg[:nblk]
        finally:
            for b in (d_stream, d_blk, d_run, d_out, d_bl, d_rl, d_st, d_pk, d_po) + ((d_bs,) if seg else ()):
                b.free()
        return out, blk_len, run_len, status

    def lz4_decompress_blocks_par(self, stream: bytes, blocks, runs, out_bytes, history=b"", pack=False, blk_fill=0):
        """gpumt_lz4_decompress_blocks_par, the same call with the blocks of a linked run decoded side by side: the
        arguments and results of lz4_decompress_blocks"""
        return self.lz4_decompress_blocks(stream, blocks, runs, out_bytes, history, pack, blk_fill,
                                          call="gpumt_lz4_decompress_blocks_par")

    def lz4_decompress_blocks_seg(self, stream: bytes, blocks, runs, out_bytes, history=b"", pack=False, blk_fill=0):
        """gpumt_lz4_decompress_blocks_seg, the same call with every block decoded in segments side by side: the arguments
        of lz4_decompress_blocks -> (out, blk_len, run_len, status, block_seg[nblk])"""
        return self.lz4_decompress_blocks(stream, blocks, runs, out_bytes, history, pack, blk_fill,
                                          call="gpumt_lz4_decompress_blocks_seg")

    def xxh32_carry(self, data: bytes, pieces):
        """XXH32 of `data` continued over `pieces` (lengths that add up to len(data)), one gpumt_xxh32_carry call per piece
        with the state carried on the device -> digest"""
        assert sum(pieces) == len(data) and pieces
        d_data = self.upload(data) if data else self.alloc(64)
        d_states, d_dig, d_ver, d_job = self.alloc(96), self.alloc(4), self.alloc(4), self.alloc(XXH32_JOB.itemsize)
        try:
            at, xs = 0, 0
            for i, n in enumerate(pieces):
                last = i == len(pieces) - 1
                job = np.zeros(1, XXH32_JOB)
                job["off"], job["len"] = at, n
                job["flags"] = (XXH_RESET if i == 0 else xs << 8) | (XXH_FINAL if last else (xs ^ 1) << 9)
                if not last:
                    xs ^= 1
                self._ck(self.L.gpumt_memcpy_h2d(self.h, d_job.ptr, job.ctypes.data, job.nbytes, 0), "h2d")
                self.sync(0)
                self._ck(self.L.gpumt_xxh32_carry(self.h, d_data.ptr, len(data), d_job.ptr, 1, d_states.ptr, d_dig.ptr,
                                                  d_ver.ptr, 0), "xxh32_carry")
                at += n
            return int(self.download(d_dig, 4, np.uint32)[0])
        finally:
            for b in (d_data, d_states, d_dig, d_ver, d_job):
                b.free()

    def zstd_decompress_blocks(self, stream: bytes, blocks, runs, out_bytes, history=b"", carry=None):
        """gpumt_zstd_decompress_blocks over host bytes: `blocks` / `runs` are ZSTD_BLOCK / ZSTD_RUN arrays, `history` is
        placed at the start of the output (what a continued run reads in front of its out_off), `carry` the 2 x
        ZSTD_CARRY_BYTES an earlier call left (None: garbage).  -> (output area bytes, run_len[nrun], status[nrun],
        carry bytes)"""
        blocks = np.ascontiguousarray(blocks, ZSTD_BLOCK)
        runs = np.ascontiguousarray(runs, ZSTD_RUN)
        nblk, nrun = len(blocks), len(runs)
        area = np.full(int(out_bytes) + 64, 0xCC, np.uint8)
        area[:len(history)] = np.frombuffer(history, np.uint8)
        cy = np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8) if carry is None else np.frombuffer(carry, np.uint8)
        d_stream = self.upload(stream) if stream else self.alloc(320)
        d_blk, d_run, d_out = self.upload(blocks.view(np.uint8)), self.upload(runs.view(np.uint8)), self.upload(area, slack=0)
        d_cy, d_rl, d_st = self.upload(cy), self.alloc(nrun * 4), self.alloc(nrun * 4)
        try:
            self._ck(self.L.gpumt_zstd_decompress_blocks(self.h, d_stream.ptr, len(stream), d_blk.ptr, nblk, d_run.ptr, nrun,
                                                         d_out.ptr, int(out_bytes), d_cy.ptr, d_rl.ptr, d_st.ptr, 0),
                     "zstd_decompress_blocks")
            status = self.download(d_st, nrun * 4, np.uint32)
            run_len = self.download(d_rl, nrun * 4, np.uint32)
            raw = self.download(d_out, int(out_bytes) + 64)
            cy_out = self.download(d_cy, 2 * ZSTD_CARRY_BYTES).tobytes()
        finally:
            for b in (d_stream, d_blk, d_run, d_out, d_cy, d_rl, d_st):
                b.free()
        assert (raw[int(out_bytes):] == 0xCC).all(), "decoder wrote past the end of its output"
        return raw[:int(out_bytes)].tobytes(), run_len, status, cy_out

    def zstd_decompress_blocks_pre(self, stream: bytes, blocks, runs, out_bytes, history=b"", carry=None):
        """gpumt_zstd_decompress_blocks_pre, the same call behind the block-parallel entropy pre-pass, with
        zstd_decompress_blocks's arguments -> (output area bytes, run_len[nrun], status[nrun], carry bytes, mark[nblk])"""
        blocks = np.ascontiguousarray(blocks, ZSTD_BLOCK)
        runs = np.ascontiguousarray(runs, ZSTD_RUN)
        nblk, nrun = len(blocks), len(runs)
        area = np.full(int(out_bytes) + 64, 0xCC, np.uint8)
        area[:len(history)] = np.frombuffer(history, np.uint8)
        cy = np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8) if carry is None else np.frombuffer(carry, np.uint8)
        d_stream = self.upload(stream) if stream else self.alloc(320)
        d_blk, d_run, d_out = self.upload(blocks.view(np.uint8)), self.upload(runs.view(np.uint8)), self.upload(area, slack=0)
        d_cy, d_rl, d_st, d_mk = self.upload(cy), self.alloc(nrun * 4), self.alloc(nrun * 4), self.alloc(max(nblk, 1) * 4)
        try:
            self._ck(self.L.gpumt_zstd_decompress_blocks_pre(self.h, d_stream.ptr, len(stream), d_blk.ptr, nblk, d_run.ptr,
                                                             nrun, d_out.ptr, int(out_bytes), d_cy.ptr, d_rl.ptr, d_st.ptr,
                                                             d_mk.ptr, 0), "zstd_decompress_blocks_pre")
            status = self.download(d_st, nrun * 4, np.uint32)
            run_len = self.download(d_rl, nrun * 4, np.uint32)
            mark = self.download(d_mk, nblk * 4, np.uint32) if nblk else np.zeros(0, np.uint32)
            raw = self.download(d_out, int(out_bytes) + 64)
            cy_out = self.download(d_cy, 2 * ZSTD_CARRY_BYTES).tobytes()
        finally:
            for b in (d_stream, d_blk, d_run, d_out, d_cy, d_rl, d_st, d_mk):
                b.free()
        assert (raw[int(out_bytes):] == 0xCC).all(), "decoder wrote past the end of its output"
        return raw[:int(out_bytes)].tobytes(), run_len, status, cy_out, mark

    def zstd_decompress_blocks_par(self, stream: bytes, blocks, runs, out_bytes, history=b"", carry=None):
        """gpumt_zstd_decompress_blocks_par, the same call with the block-parallel execute stage behind the entropy
        pre-pass, with zstd_decompress_blocks's arguments -> (output area bytes, run_len[nrun], status[nrun], carry bytes,
        mark[nblk], par[nblk])"""
        blocks = np.ascontiguousarray(blocks, ZSTD_BLOCK)
        runs = np.ascontiguousarray(runs, ZSTD_RUN)
        nblk, nrun = len(blocks), len(runs)
        area = np.full(int(out_bytes) + 64, 0xCC, np.uint8)
        area[:len(history)] = np.frombuffer(history, np.uint8)
        cy = np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8) if carry is None else np.frombuffer(carry, np.uint8)
        d_stream = self.upload(stream) if stream else self.alloc(320)
        d_blk, d_run, d_out = self.upload(blocks.view(np.uint8)), self.upload(runs.view(np.uint8)), self.upload(area, slack=0)
        d_cy, d_rl, d_st = self.upload(cy), self.alloc(nrun * 4), self.alloc(nrun * 4)
        d_mk, d_pr = self.alloc(max(nblk, 1) * 4), self.alloc(max(nblk, 1) * 4)
        try:
            self._ck(self.L.gpumt_zstd_decompress_blocks_par(self.h, d_stream.ptr, len(stream), d_blk.ptr, nblk, d_run.ptr,
                                                             nrun, d_out.ptr, int(out_bytes), d_cy.ptr, d_rl.ptr, d_st.ptr,
                                                             d_mk.ptr, d_pr.ptr, 0), "zstd_decompress_blocks_par")
            status = self.download(d_st, nrun * 4, np.uint32)
            run_len = self.download(d_rl, nrun * 4, np.uint32)
            mark = self.download(d_mk, nblk * 4, np.uint32) if nblk else np.zeros(0, np.uint32)
            par = self.download(d_pr, nblk * 4, np.uint32) if nblk else np.zeros(0, np.uint32)
            raw = self.download(d_out, int(out_bytes) + 64)
            cy_out = self.download(d_cy, 2 * ZSTD_CARRY_BYTES).tobytes()
        finally:
            for b in (d_stream, d_blk, d_run, d_out, d_cy, d_rl, d_st, d_mk, d_pr):
                b.free()
        assert (raw[int(out_bytes):] == 0xCC).all(), "decoder wrote past the end of its output"
        return raw[:int(out_bytes)].tobytes(), run_len, status, cy_out, mark, par

    def xxh64_carry(self, data: bytes, pieces):
        """low 32 bits of XXH64 of `data` continued over `pieces` (lengths that add up to len(data)), one gpumt_xxh64_carry
        call per piece with the state carried on the device -> digest"""
        assert sum(pieces) == len(data) and pieces
        d_data = self.upload(data) if data else self.alloc(64)
        d_states, d_dig, d_ver = self.alloc(2 * XXH64_STATE_WORDS * 4), self.alloc(4), self.alloc(4)
        d_job = self.alloc(XXH32_JOB.itemsize)
        try:
            at, xs = 0, 0
            for i, n in enumerate(pieces):
                last = i == len(pieces) - 1
                job = np.zeros(1, XXH32_JOB)
                job["off"], job["len"] = at, n
                job["flags"] = (XXH_RESET if i == 0 else xs << 8) | (XXH_FINAL if last else (xs ^ 1) << 9)
                if not last:
                    xs ^= 1
                self._ck(self.L.gpumt_memcpy_h2d(self.h, d_job.ptr, job.ctypes.data, job.nbytes, 0), "h2d")
                self.sync(0)
                self._ck(self.L.gpumt_xxh64_carry(self.h, d_data.ptr, len(data), d_job.ptr, 1, d_states.ptr, d_dig.ptr,
                                                  d_ver.ptr, 0), "xxh64_carry")
                at += n
            return int(self.download(d_dig, 4, np.uint32)[0])
        finally:
            for b in (d_data, d_states, d_dig, d_ver, d_job):
                b.free()

    def zstd_slot_stride(self, chunk):
        return int(self.L.gpumt_zstd_slot_stride(chunk))

    def zstd_compress(self, d_in, n, chunk, d_slots, stride, d_rec_len, stream=0, level=1, win=False):
        """win=True: gpumt_zstd_compress_batch_win, the whole chunk as the match window from level 10 on"""
        call = self.L.gpumt_zstd_compress_batch_win if win else self.L.gpumt_zstd_compress_batch_level
        self._ck(call(self.h, d_in.ptr, int(n), int(chunk), d_slots.ptr, int(stride), d_rec_len.ptr, int(level), stream),
                 "zstd_compress_batch_win" if win else "zstd_compress_batch_level")

    def zstd_win_depth(self, level):
        return int(self.L.gpumt_zstd_win_depth(int(level)))

    def win_chain_plane(self, data: bytes, chunk, seg_log=0):
        """gpumt_win_chain_plane over host bytes -> the chain plane of the window encoders, one u32 per byte; seg_log 0 =
        one wave per chunk, 12..24 = in segments of 1 << seg_log positions.  Refused head tables raise NativeError"""
        n = len(data)
        d_in = self.upload(data)
        d_pl = self.upload(np.full(n + 1, 0xA5A5A5A5, np.uint32), slack=0)
        try:
            self._ck(self.L.gpumt_win_chain_plane(self.h, d_in.ptr, n, int(chunk), d_pl.ptr, int(seg_log), 0), "win_chain_plane")
            plane = self.download(d_pl, 4 * (n + 1), np.uint32)
        finally:
            d_in.free()
            d_pl.free()
        assert int(plane[n]) == 0xA5A5A5A5, "the chain build wrote past the end of the plane"
        return plane[:n]

    def win_chain_par_scratch(self, n, chunk, seg_log):
        return int(self.L.gpumt_win_chain_par_scratch(int(n), int(chunk), int(seg_log)))

    def zstd_probe(self, d_stream, d_rec_off, d_rec_len, nrec, d_out_len, d_out_off, d_status, stream=0):
        self._ck(self.L.gpumt_zstd_probe_sizes(self.h, d_stream.ptr, d_rec_off.ptr, d_rec_len.ptr, nrec,
                                               d_out_len.ptr, d_out_off.ptr, d_status.ptr, stream),
                 "zstd_probe_sizes")

    def zstd_decompress(self, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes,
                        d_out_off, d_out_len, d_status, stream=0):
        self._ck(self.L.gpumt_zstd_decompress_batch(self.h, d_stream.ptr, int(stream_bytes),
                                                    d_rec_off.ptr, d_rec_len.ptr, nrec, d_out.ptr,
                                                    int(out_bytes), d_out_off.ptr, d_out_len.ptr,
                                                    d_status.ptr, stream), "zstd_decompress_batch")

    def zstd_decompress_par(self, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes,
                            d_out_off, d_out_len, d_status, d_rec_par=None, stream=0):
        """gpumt_zstd_decompress_batch_par: zstd_decompress with the records of several blocks decoded block-parallel;
        d_rec_par (nrec words, may be None) receives per record the blocks that route decoded and kept"""
        self._ck(self.L.gpumt_zstd_decompress_batch_par(self.h, d_stream.ptr, int(stream_bytes), d_rec_off.ptr,
                                                        d_rec_len.ptr, nrec, d_out.ptr, int(out_bytes), d_out_off.ptr,
                                                        d_out_len.ptr, d_status.ptr,
                                                        d_rec_par.ptr if d_rec_par is not None else None, stream),
                 "zstd_decompress_batch_par")

    def zstd_decompress_par_bytes(self, stream: bytes, rec_off, rec_len):
        """decompress_bytes for zstd-mt records through zstd_decompress_par -> (content bytes, status[n], rec_par[n])"""
        nrec = len(rec_len)
        d_stream = self.upload(stream)
        d_ro = self.upload(np.asarray(rec_off, np.uint64)[:nrec].copy())
        d_rl = self.upload(np.asarray(rec_len, np.uint32).copy())
        d_ol, d_oo, d_st, d_rp = self.alloc(nrec * 4), self.alloc((nrec + 1) * 8), self.alloc(nrec * 4), self.alloc(nrec * 4)
        try:
            self.zstd_probe(d_stream, d_ro, d_rl, nrec, d_ol, d_oo, d_st)
            total = int(self.download(d_oo, (nrec + 1) * 8, np.uint64)[nrec])
            d_out = self.alloc(total + 64)
            try:
                lib().gpumt_memset(self.h, d_out.ptr, 0xCC, total + 64, 0)
                self.zstd_decompress_par(d_stream, len(stream), d_ro, d_rl, nrec, d_out, total, d_oo, d_ol, d_st, d_rp)
                status = self.download(d_st, nrec * 4, np.uint32)
                rec_par = self.download(d_rp, nrec * 4, np.uint32)
                raw = self.download(d_out, total + 64)
                assert (raw[total:] == 0xCC).all(), "decoder wrote past the end of its output"
            finally:
                d_out.free()
        finally:
            for b in (d_stream, d_ro, d_rl, d_ol, d_oo, d_st, d_rp):
                b.free()
        return raw[:total].tobytes(), status, rec_par

    def brotli_compress(self, d_in, n, chunk, d_slots, stride, d_rec_len, stream=0, level=1, win=False, index=False):
        """win=True: gpumt_brotli_compress_batch_win, the whole chunk as the match window from quality 9 on;
        index=True: gpumt_brotli_compress_batch_index, the table encoders' records with a span index"""
        assert not (win and index), "the window encoder writes no index"
        name = "brotli_compress_batch_" + ("win" if win else "index" if index else "level")
        call = getattr(self.L, "gpumt_" + name)
        self._ck(call(self.h, d_in.ptr, int(n), int(chunk), d_slots.ptr, int(stride), d_rec_len.ptr, int(level), stream), name)

    def brotli_win_depth(self, level):
        return int(self.L.gpumt_brotli_win_depth(int(level)))

    def brotli_decompress(self, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len,
                          d_status, stream=0):
        self._ck(self.L.gpumt_brotli_decompress_batch(self.h, d_stream.ptr, d_rec_off.ptr, d_rec_len.ptr, nrec,
                                                      d_out.ptr, d_out_off.ptr, d_out_cap.ptr, d_out_len.ptr,
                                                      d_status.ptr, stream), "brotli_decompress_batch")

    def brotli_decompress_par(self, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len,
                              d_status, d_rec_par, stream=0):
        """gpumt_brotli_decompress_batch_par: indexed records span by span, the rest by the record decoders"""
        self._ck(self.L.gpumt_brotli_decompress_batch_par(self.h, d_stream.ptr, d_rec_off.ptr, d_rec_len.ptr, nrec,
                                                          d_out.ptr, d_out_off.ptr, d_out_cap.ptr, d_out_len.ptr,
                                                          d_status.ptr, d_rec_par.ptr if d_rec_par is not None else None,
                                                          stream), "brotli_decompress_batch_par")

    # snappy-mt (include/gpumt.h gpumt_snappy_*): same call shapes as brotli
    def snappy_slot_stride(self, chunk):
        return int(self.L.gpumt_snappy_slot_stride(int(chunk)))

    def snappy_compress(self, d_in, n, chunk, d_slots, stride, d_rec_len, stream=0):
        self._ck(self.L.gpumt_snappy_compress_batch(self.h, d_in.ptr, int(n), int(chunk), d_slots.ptr,
                                                    int(stride), d_rec_len.ptr, stream), "snappy_compress_batch")

    def snappy_decompress(self, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len,
                          d_status, stream=0):
        self._ck(self.L.gpumt_snappy_decompress_batch(self.h, d_stream.ptr, d_rec_off.ptr, d_rec_len.ptr, nrec,
                                                      d_out.ptr, d_out_off.ptr, d_out_cap.ptr, d_out_len.ptr,
                                                      d_status.ptr, stream), "snappy_decompress_batch")

    def brotli_decompress_bytes(self, stream: bytes, rec_off, rec_len, cap):
        """Records of a brotli-mt stream (payload offsets / sizes / capacities as the host engine
        parses them) -> (list of decoded records, status[n])"""
        nrec = len(rec_off)
        out_off = np.zeros(nrec + 1, np.uint64)
        out_off[1:] = np.cumsum(np.asarray(cap, np.uint64))
        total = int(out_off[nrec])
        d_stream = self.upload(stream + b"\0" * 256)
        d_ro, d_rl = self.upload(np.asarray(rec_off, np.uint64).copy()), self.upload(np.asarray(rec_len, np.uint32).copy())
        d_oo, d_oc = self.upload(out_off), self.upload(np.asarray(cap, np.uint32).copy())
        d_ol, d_st = self.alloc(nrec * 4), self.alloc(nrec * 4)
        d_out = self.upload(np.full(total + 64, 0xCC, np.uint8))
        try:
            self.brotli_decompress(d_stream, d_ro, d_rl, nrec, d_out, d_oo, d_oc, d_ol, d_st)
            status = self.download(d_st, nrec * 4, np.uint32)
            out_len = self.download(d_ol, nrec * 4, np.uint32)
            raw = self.download(d_out, total + 64)
        finally:
            for b in (d_stream, d_ro, d_rl, d_oo, d_oc, d_ol, d_st, d_out):
                b.free()
        assert (raw[total:] == 0xCC).all(), "decoder wrote past the end of its output"
        recs = []
        for i in range(nrec):
            o, n = int(out_off[i]), int(out_len[i])
            assert n <= int(cap[i])
            if status[i] == 0:
                assert (raw[o + n:o + int(cap[i])] == 0xCC).all(), "wrote past the decoded size"
            recs.append(raw[o:o + n].tobytes())
        return recs, status

    def brotli_decompress_par_bytes(self, stream: bytes, rec_off, rec_len, cap, out_off=None, par=True):
        """brotli_decompress_bytes through gpumt_brotli_decompress_batch_par -> (list of decoded records, status[n],
        out_len[n], rec_par[n]).  out_off: where each record's output area starts (default: back to back); every byte
        outside the areas must come back untouched.  par=False: the serial call in the same layout (rec_par all 0)."""
        nrec = len(rec_off)
        cap = np.asarray(cap, np.uint32)
        if out_off is None:
            out_off = np.zeros(nrec, np.uint64)
            out_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
        out_off = np.asarray(out_off, np.uint64)
        total = max(int(o) + int(c) for o, c in zip(out_off, cap))
        d_stream = self.upload(stream + b"\0" * 256)
        d_ro, d_rl = self.upload(np.asarray(rec_off, np.uint64).copy()), self.upload(np.asarray(rec_len, np.uint32).copy())
        d_oo, d_oc = self.upload(out_off.copy()), self.upload(cap.copy())
        d_ol, d_st = self.upload(np.full(nrec, 0xFFFFFFFF, np.uint32)), self.upload(np.full(nrec, 99, np.uint32))
        d_rp = self.upload(np.full(nrec, 7, np.uint32))
        d_out = self.upload(np.full(total + 64, 0xCC, np.uint8))
        try:
            if par:
                self.brotli_decompress_par(d_stream, d_ro, d_rl, nrec, d_out, d_oo, d_oc, d_ol, d_st, d_rp)
                rec_par = self.download(d_rp, nrec * 4, np.uint32)
            else:
                self.brotli_decompress(d_stream, d_ro, d_rl, nrec, d_out, d_oo, d_oc, d_ol, d_st)
                rec_par = np.zeros(nrec, np.uint32)
            status = self.download(d_st, nrec * 4, np.uint32)
            out_len = self.download(d_ol, nrec * 4, np.uint32)
            raw = self.download(d_out, total + 64)
        finally:
            for b in (d_stream, d_ro, d_rl, d_oo, d_oc, d_ol, d_st, d_rp, d_out):
                b.free()
        inside = np.zeros(total + 64, bool)
        recs = []
        for i in range(nrec):
            o, n = int(out_off[i]), int(out_len[i]) if status[i] == 0 else 0
            assert n <= int(cap[i])
            inside[o:o + int(cap[i])] = True
            if status[i] == 0:
                assert (raw[o + n:o + int(cap[i])] == 0xCC).all(), "wrote past the decoded size"
            recs.append(raw[o:o + n].tobytes())
        assert (raw[~inside] == 0xCC).all(), "decoder wrote outside the records' output areas"
        return recs, status, out_len, rec_par

    # ---- convenience round trips on host bytes (tests) ----------------------------------------
    def compress_bytes(self, data: bytes, chunk: int, codec="lz4", level=1, win=False, index=False):
        """-> (stream bytes, rec_off[n+1] u64, rec_len[n] u32); win: codec "zstd" or "brotli" with the whole-chunk window;
        index: codec "brotli" with the span index of gpumt_brotli_compress_batch_index"""
        assert not win or codec in ("zstd", "brotli")
        assert not index or codec == "brotli"
        n = len(data)
        nrec = self.record_count(n, chunk)
        stride = self.zstd_slot_stride(chunk) if codec in ("zstd", "brotli") else self.slot_stride(chunk)
        d_in = self.upload(data)
        d_slots = self.alloc(nrec * stride)
        d_len = self.alloc(nrec * 4)
        d_off = self.alloc((nrec + 1) * 8)
        try:
            if codec == "zstd":
                self.zstd_compress(d_in, n, chunk, d_slots, stride, d_len, level=level, win=win)
            elif codec == "brotli":
                self.brotli_compress(d_in, n, chunk, d_slots, stride, d_len, level=level, win=win, index=index)
            else:
                self.lz4_compress(d_in, n, chunk, d_slots, stride, d_len, level=level)
            rec_len = self.download(d_len, nrec * 4, np.uint32)
            total = int(rec_len.astype(np.uint64).sum())
            d_stream = self.alloc(total + 64)
            try:
                self.lz4_compact(d_slots, stride, d_len, nrec, d_stream, d_off)
                rec_off = self.download(d_off, (nrec + 1) * 8, np.uint64)
                assert int(rec_off[nrec]) == total
                stream = self.download(d_stream, total).tobytes()
            finally:
                d_stream.free()
        finally:
            for b in (d_in, d_slots, d_len, d_off):
                b.free()
        return stream, rec_off, rec_len

    def decompress_bytes(self, stream: bytes, rec_off, rec_len, codec="lz4"):
        """-> (content bytes, status[n])"""
        nrec = len(rec_len)
        d_stream = self.upload(stream)
        d_ro = self.upload(np.asarray(rec_off, np.uint64)[:nrec].copy())
        d_rl = self.upload(np.asarray(rec_len, np.uint32).copy())
        d_ol = self.alloc(nrec * 4)
        d_oo = self.alloc((nrec + 1) * 8)
        d_st = self.alloc(nrec * 4)
        try:
            if codec == "zstd":
                self.zstd_probe(d_stream, d_ro, d_rl, nrec, d_ol, d_oo, d_st)
            else:
                self.lz4_probe(d_stream, d_ro, d_rl, nrec, d_ol, d_oo)
            out_off = self.download(d_oo, (nrec + 1) * 8, np.uint64)
            total = int(out_off[nrec])
            d_out = self.alloc(total + 64)
            try:
                lib().gpumt_memset(self.h, d_out.ptr, 0xCC, total + 64, 0)
                if codec == "zstd":
                    self.zstd_decompress(d_stream, len(stream), d_ro, d_rl, nrec, d_out, total, d_oo, d_ol, d_st)
                else:
                    self.lz4_decompress(d_stream, len(stream), d_ro, d_rl, nrec, d_out, total, d_oo, d_ol, d_st)
                status = self.download(d_st, nrec * 4, np.uint32)
                raw = self.download(d_out, total + 64)
                assert (raw[total:] == 0xCC).all(), "decoder wrote past the end of its output"
                out = raw[:total].tobytes()
            finally:
                d_out.free()
        finally:
            for b in (d_stream, d_ro, d_rl, d_ol, d_oo, d_st):
                b.free()
        return out, status
