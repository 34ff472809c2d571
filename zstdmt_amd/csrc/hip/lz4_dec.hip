/*
 * lz4_dec.hip -- LZ4 frame decoder, one wave per record (= one chunk).
 *
 * Replaces, per record, LZ4F_decompress (call site /root/reference/lib/lz4-mt_decompress.c:349-362)
 * together with the record checks of pt_read (:229-236): skippable magic and length, LZ4F magic /
 * version / reserved bits / header checksum, block walk (stored or LZ4 block with the chunk's
 * earlier output as prefix -- linked blocks), end mark, content size.  The XXH32 content checksum
 * is extracted here and verified by zmt_xxh32_kernel over the decoded bytes.
 *
 * Variant "serial" (this file, kernel zmt_lz4_dec_serial): the token stream is walked
 * wave-uniformly, the 64 lanes cooperate on each literal run and each match (byte i of the copy
 * is lane i mod 64).  Overlapping matches (offset < length) read the pattern's first period, so a
 * copy never depends on bytes written by the same sequence.  Output is written straight to HBM;
 * match sources are read back through L1/L2 (same wave, program order).
 */
#include "lz4_common.h"
#include "lz4_frame.h"

/*
 * Decode one LZ4 block [src, src+slen) appending at out[opos...]; matches may reach back to
 * out[low].  Returns new opos or 0xFFFFFFFF on malformed input.  limit = highest legal opos,
 * blkmax = the frame's block maximum: liblz4's end-of-block rules (lz4lib_tail_bad, lz4_common.h)
 * are measured from it.
 */
static __device__ u32 decode_block_serial(const u8 *src, u32 slen, u8 *out, u32 opos, u32 low,
					  u32 limit, u32 blkmax, int lane)
{
	u32 ip = 0;
	const u32 opos0 = opos;
	if (slen == 0)
		return 0xFFFFFFFFu;
	for (;;) {
		u32 tok, lit, ml, off, t;
		if (ip >= slen)
			return 0xFFFFFFFFu;
		t = ip;
		tok = uld8(src + ip++);
		lit = tok >> 4;
		if (lit == 15) {
			u32 b;
			if (slen - ip <= 15)
				return 0xFFFFFFFFu;
			do {
				if (ip >= slen)
					return 0xFFFFFFFFu;
				b = uld8(src + ip++);
				lit += b;
			} while (b == 255);
		}
		if (slen - ip < lit || limit - opos < lit)
			return 0xFFFFFFFFu;
		if (slen - ip > lit && lz4lib_tail_bad(t, ip, lit, opos - opos0, slen, blkmax))
			return 0xFFFFFFFFu;
		wave_copy(out + opos, src + ip, lit, lane);
		ip += lit;
		opos += lit;
		if (ip == slen)
			return opos;
		if (slen - ip < 2)
			return 0xFFFFFFFFu;
		off = uld16(src + ip);
		ip += 2;
		ml = tok & 15;
		if (ml == 15) {
			u32 b;
			do {
				if (ip >= slen)
					return 0xFFFFFFFFu;
				b = uld8(src + ip++);
				ml += b;
			} while (b == 255);
			if (slen - ip < 5)
				return 0xFFFFFFFFu;
		}
		ml += 4;
		if (off == 0 || off > opos - low || limit - opos < ml)
			return 0xFFFFFFFFu;
		if (lz4lib_match_tail_bad(t, tok, off, opos - opos0 - lit, lit + ml, slen, blkmax))
			return 0xFFFFFFFFu;
		wave_mem_fence();
		{
			const u8 *m = out + opos - off;
			u8 *d = out + opos;
			if (off >= ml) {
				for (u32 i = (u32)lane; i < ml; i += 64)
					d[i] = m[i];
			} else {
				/* periodic fill: byte i of the match equals byte i mod off of the source */
				for (u32 i = (u32)lane; i < ml; i += 64)
					d[i] = m[i % off];
			}
		}
		opos += ml;
	}
}

/* XXH32 (seed 0) of [p, p + len) by one wave: lanes 0..3 carry the four accumulators over the
 * 16-byte stripes, lane 0 folds the tail; the result is wave-uniform */
static __device__ u32 wave_xxh32(const u8 *p, u32 len, int lane)
{
	u32 v = 0;
	if (len >= 16 && lane < 4) {
		u32 acc = (lane == 0) ? XP1 + XP2 : (lane == 1) ? XP2 : (lane == 2) ? 0u : 0u - XP1;
		const u8 *q = p + lane * 4;
		for (u32 s = 0, ns = len >> 4; s < ns; s++) {
			acc = xxh_round(acc, ld32u(q));
			q += 16;
		}
		v = rotl32(acc, (lane == 0) ? 1 : (lane == 1) ? 7 : (lane == 2) ? 12 : 18);
	}
	v += wv_shfl(v, lane ^ 1);
	v += wv_shfl(v, lane ^ 2);
	u32 h = (len >= 16 ? v : XP5) + len;
	if (lane == 0)
		h = xxh_tail(h, p + (len & ~15u), len & 15);
	return wv_readlane(h, 0);
}

static __device__ __forceinline__ void
lz4_dec_serial_body(const u8 *__restrict__ stream, const u64 *__restrict__ rec_off,
		    const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base,
		    const u64 *__restrict__ out_off, u32 *__restrict__ out_len,
		    u32 *__restrict__ status, u32 *__restrict__ chk_expect,
		    u32 *__restrict__ chk_valid, u32 only_status,
		    const u32 *__restrict__ kept) /* NULL, or per record ST_REC_KEPT = pass it by */
{
	const u32 rec = blockIdx.x;
	const int lane = wv_lane();
	if (rec >= nrec)
		return;
	/* clean-up pass of the split decoder: only records it flagged for this kernel */
	if (only_status != 0xFFFFFFFFu && wv_readfirst(status[rec]) != only_status)
		return;
	if (kept && wv_readfirst(kept[rec]) == ST_REC_KEPT) {
		if (lane == 0)
			status[rec] = ST_REC_KEPT; /* (as zmt_dec_frames_kept_kernel: the caller's merge reads it as "passed by") */
		return;
	}
	const u8 *r = stream + rec_off[rec];
	const u32 rlen = rec_len[rec];
	u8 *out = out_base + out_off[rec];
	const u32 cap = out_len[rec];
	u32 st = ST_OK, opos = 0, ip, flen;
	FrameInfo fi;

	if (lane == 0) {
		chk_valid[rec] = 0;
		chk_expect[rec] = 0;
	}
	if (rlen < 12 || uld32(r) != ZMT_SKIP_MAGIC || uld32(r + 4) != 4 ||
	    uld32(r + 8) != rlen - 12) {
		st = ST_BAD_RECORD;
		goto done;
	}
	flen = rlen - 12;
	r += 12;
	st = parse_frame_header(r, flen, fi);
	if (st != ST_OK)
		goto done;
	ip = fi.hdr;
	for (;;) {
		u32 bh, bsz;
		if (flen - ip < 4) {
			st = ST_BAD_BLOCK;
			goto done;
		}
		bh = uld32(r + ip);
		ip += 4;
		if (bh == 0)
			break;
		bsz = bh & 0x7FFFFFFFu;
		if (bsz > fi.blkmax || flen - ip < bsz || (fi.has_bcheck && flen - ip - bsz < 4)) {
			st = ST_BAD_BLOCK;
			goto done;
		}
		if (fi.has_bcheck && wave_xxh32(r + ip, bsz, lane) != uld32(r + ip + bsz)) {
			st = ST_BAD_CHECKSUM; /* LZ4F_ERROR_blockChecksum_invalid */
			goto done;
		}
		if (bh & 0x80000000u) {
			if (cap - opos < bsz) {
				st = ST_BAD_BLOCK;
				goto done;
			}
			wave_copy(out + opos, r + ip, bsz, lane);
			opos += bsz;
		} else {
			u32 room = cap - opos < fi.blkmax ? cap - opos : fi.blkmax;
			u32 np = decode_block_serial(r + ip, bsz, out, opos, fi.indep ? opos : 0,
						     opos + room, fi.blkmax, lane);
			if (np == 0xFFFFFFFFu) {
				st = ST_BAD_BLOCK;
				goto done;
			}
			opos = np;
		}
		ip += bsz + (fi.has_bcheck ? 4u : 0u);
	}
	/* a frame that states its content size must produce exactly that (= out_len); one that does not
	 * (plain .lz4 files of the lz4 tool; never lz4-mt) was given a capacity and reports its size */
	if (fi.has_csize ? (fi.csize != (u64)opos || opos != cap) : opos > cap) {
		st = ST_SIZE_MISMATCH;
		goto done;
	}
	if (!fi.has_csize && lane == 0)
		out_len[rec] = opos;
	if (fi.has_ccheck) {
		if (flen - ip < 4) {
			st = ST_BAD_BLOCK;
			goto done;
		}
		if (lane == 0) {
			chk_expect[rec] = ld32u(r + ip);
			chk_valid[rec] = 1;
		}
		ip += 4;
	}
	if (ip != flen)
		st = ST_TRAILING;
done:
	if (lane == 0)
		status[rec] = st;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_dec_serial(const u8 *__restrict__ stream, const u64 *__restrict__ rec_off,
		   const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base,
		   const u64 *__restrict__ out_off, u32 *__restrict__ out_len,
		   u32 *__restrict__ status, u32 *__restrict__ chk_expect,
		   u32 *__restrict__ chk_valid, u32 only_status)
{
	lz4_dec_serial_body(stream, rec_off, rec_len, nrec, out_base, out_off, out_len, status, chk_expect, chk_valid, only_status,
			    nullptr);
}

/* the same kernel for gpumt_lz4_decompress_batch_par's record pass: records whose kept word is ST_REC_KEPT are passed by */
extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_dec_serial_kept(const u8 *__restrict__ stream, const u64 *__restrict__ rec_off,
			const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base,
			const u64 *__restrict__ out_off, u32 *__restrict__ out_len,
			u32 *__restrict__ status, u32 *__restrict__ chk_expect,
			u32 *__restrict__ chk_valid, u32 only_status, const u32 *__restrict__ kept)
{
	lz4_dec_serial_body(stream, rec_off, rec_len, nrec, out_base, out_off, out_len, status, chk_expect, chk_valid, only_status,
			    kept);
}

/*
 * Block-level entry (gpumt_lz4_decompress_blocks): the plain .lz4 path of the host engine walks the frame and block
 * headers itself and hands over a table of blocks and a list of runs.  A run is a group of consecutive blocks that one
 * wave decodes back to back from out_base + out_off: one block of an independent-block frame (low = out_off), or the
 * blocks a linked-block frame has in this batch (low reaches back over the history the caller placed in front, at
 * most 64 KiB: LZ4 offsets are 16 bits).  Order inside a run comes from the run being one wave; no run looks at
 * another's memory.  The table entries live in device memory, so they are checked here against the sizes the host
 * passed: an entry that leaves the stream or the output is ST_BAD_RECORD and nothing of it is touched.
 * Verdicts as zmt_lz4_dec_serial: ST_BAD_BLOCK (malformed, above the block maximum, no room), ST_BAD_CHECKSUM.
 */
struct Lz4Block { /* == gpumt_lz4_block */
	u64 src_off;
	u32 src_len, flags, blkmax, checksum;
};
struct Lz4Run { /* == gpumt_lz4_run */
	u64 low, out_off;
	u32 out_cap, first, count, reserved;
};
#define LZ4B_STORED 1u
#define LZ4B_CHECKSUM 2u

/* the checks of a run's table entry against the sizes the host passed */
static __device__ __forceinline__ bool lz4_run_ok(const Lz4Run &R, u32 nblk, u64 out_bytes)
{
	return !(R.first > nblk || R.count > nblk - R.first || R.low > R.out_off || R.out_off > out_bytes ||
		 R.out_cap > out_bytes - R.out_off || R.out_off - R.low > 0x10000u || R.out_cap > 0xFFFE0000u);
}

/* one wave decodes run r, block after block */
static __device__ void lz4_run_serial(const u8 *__restrict__ stream, u64 stream_bytes, const Lz4Block *__restrict__ blocks,
				      u32 nblk, const Lz4Run &R, u32 r, u8 *out_base, u64 out_bytes, u32 *__restrict__ blk_len,
				      u32 *__restrict__ run_len, u32 *__restrict__ status, int lane)
{
	u32 st = ST_OK, opos = 0, start = 0;
	if (!lz4_run_ok(R, nblk, out_bytes)) {
		st = ST_BAD_RECORD;
		goto done;
	}
	{
		u8 *out = out_base + R.low;
		const u32 end = wv_readfirst((u32)(R.out_off - R.low) + R.out_cap);
		start = opos = wv_readfirst((u32)(R.out_off - R.low));
		for (u32 b = R.first; b < R.first + R.count; b++) {
			const Lz4Block B = blocks[b];
			const u32 bsz = wv_readfirst(B.src_len), bm = wv_readfirst(B.blkmax);
			const u8 *src = stream + B.src_off;
			if (B.src_off > stream_bytes || bsz > stream_bytes - B.src_off || bm < 65536u || bm > (4u << 20)) {
				st = ST_BAD_RECORD;
				break;
			}
			if (bsz > bm) {
				st = ST_BAD_BLOCK;
				break;
			}
			if ((B.flags & LZ4B_CHECKSUM) && wave_xxh32(src, bsz, lane) != wv_readfirst(B.checksum)) {
				st = ST_BAD_CHECKSUM; /* LZ4F_ERROR_blockChecksum_invalid */
				break;
			}
			u32 np;
			if (B.flags & LZ4B_STORED) {
				if (end - opos < bsz) {
					st = ST_BAD_BLOCK;
					break;
				}
				wave_copy(out + opos, src, bsz, lane);
				np = opos + bsz;
			} else {
				const u32 room = end - opos < bm ? end - opos : bm;
				np = decode_block_serial(src, bsz, out, opos, 0, opos + room, bm, lane);
				if (np == 0xFFFFFFFFu) {
					st = ST_BAD_BLOCK;
					break;
				}
			}
			if (lane == 0)
				blk_len[b] = np - opos;
			opos = np;
		}
	}
done:
	if (lane == 0) {
		run_len[r] = opos - start;
		status[r] = st;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_dec_blocks_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const Lz4Block *__restrict__ blocks, u32 nblk,
			  const Lz4Run *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes,
			  u32 *__restrict__ blk_len, u32 *__restrict__ run_len, u32 *__restrict__ status)
{
	const u32 r = blockIdx.x;
	if (r >= nrun)
		return;
	const Lz4Run R = runs[r];
	lz4_run_serial(stream, stream_bytes, blocks, nblk, R, r, out_base, out_bytes, blk_len, run_len, status, wv_lane());
}

/* run r's decoded bytes (out_base + out_off, run_len[r] of them) -> dst + off[r]: the pack of the slots of
 * independent blocks that decoded to less than their capacity (off = zmt_scan_kernel over run_len); the pattern of
 * zmt_compact_kernel with a slot table in place of a stride */
extern "C" __global__ void __launch_bounds__(256)
zmt_lz4_gather_runs_kernel(const u8 *__restrict__ out_base, u64 out_bytes, const Lz4Run *__restrict__ runs,
			   const u32 *__restrict__ run_len, const u64 *__restrict__ off, u32 nrun, u8 *__restrict__ dst,
			   u64 dst_bytes)
{
	const u32 r = blockIdx.x;
	if (r >= nrun)
		return;
	const u64 so = runs[r].out_off, dofs = off[r];
	const u32 n = run_len[r];
	if (so > out_bytes || n > out_bytes - so || dofs > dst_bytes || n > dst_bytes - dofs)
		return;
	const u8 *s = out_base + so;
	u8 *d = dst + dofs;
	for (u32 i = threadIdx.x * 4; i + 4 <= n; i += 1024)
		st32u(d + i, ld32u(s + i));
	if (threadIdx.x < (n & 3))
		d[(n & ~3u) + threadIdx.x] = s[(n & ~3u) + threadIdx.x];
}

#include "lz4_dec_par.h"
#include "lz4_dec_seg.h"
#include "lz4_dec_rec.h"

#ifdef ZMT_EMU
/*
 * TEST HARNESS ONLY (tests/emu compiles this file as host C++): the two device calls above over the fiber emulator,
 * with the shapes of include/gpumt.h, so that the host engine's plain .lz4 path runs on the CPU.  Synchronous, host
 * pointers stand in for device pointers; the same argument checks as gpumt.hip.  Never part of the product.
 */
#include <vector>
#include "../../../include/gpumt.h"
extern "C" {
void zmt_scan_kernel(const u32 *, u32, u64 *);

void emu_lz4_decompress_blocks(const u8 *stream, u64 stream_bytes, const void *blocks, u32 nblk, const void *runs,
			       u32 nrun, u8 *out, u64 out_bytes, u32 *blk_len, u32 *run_len, u32 *status)
{
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_lz4_dec_blocks_kernel(stream, stream_bytes, (const Lz4Block *)blocks, nblk, (const Lz4Run *)runs, nrun, out,
					  out_bytes, blk_len, run_len, status);
	});
}

void emu_lz4_pack_runs(const u8 *out, u64 out_bytes, const void *runs, const u32 *run_len, u32 nrun, u8 *packed,
		       u64 packed_bytes, u64 *pack_off)
{
	emu::launch(emu::dim3{1, 1, 1}, emu::dim3{1024, 1, 1}, [=]() { zmt_scan_kernel(run_len, nrun, pack_off); });
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{256, 1, 1}, [=]() {
		zmt_lz4_gather_runs_kernel(out, out_bytes, (const Lz4Run *)runs, run_len, pack_off, nrun, packed, packed_bytes);
	});
}

int gpumt_lz4_decompress_blocks(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const gpumt_lz4_block *d_blocks,
				size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun, void *d_out, size_t out_bytes,
				uint32_t *d_block_len, uint32_t *d_run_len, uint32_t *d_status, int s)
{
	static_assert(sizeof(gpumt_lz4_block) == sizeof(Lz4Block) && sizeof(gpumt_lz4_run) == sizeof(Lz4Run), "table layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_stream || !d_blocks || !d_runs || !d_out || !d_block_len || !d_run_len ||
	    !d_status || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	emu_lz4_decompress_blocks((const u8 *)d_stream, stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out,
				  out_bytes, d_block_len, d_run_len, d_status);
	return GPUMT_OK;
}

/* par_on = 0, or a table without a run of two blocks: the serial kernel (the developer knob of the real boundary) */
void emu_lz4_decompress_blocks_par(const u8 *stream, u64 stream_bytes, const void *blocks, u32 nblk, const void *runs,
				   u32 nrun, u8 *out, u64 out_bytes, u32 *blk_len, u32 *run_len, u32 *status, int par_on)
{
	if (!par_on || nblk <= nrun) {
		emu_lz4_decompress_blocks(stream, stream_bytes, blocks, nblk, runs, nrun, out, out_bytes, blk_len, run_len, status);
		return;
	}
	std::vector<u16> origin((size_t)out_bytes + 4, 0xA5A5); /* scratch starts as garbage */
	std::vector<u32> owner(nblk, LZ4P_NONE), words((size_t)4 * nblk, 0xA5A5A5A5u), flag(1, 0);
	const Lz4Par P = {origin.data(), owner.data(), words.data(), words.data() + nblk, words.data() + 2 * (size_t)nblk,
			  words.data() + 3 * (size_t)nblk, flag.data()};
	const Lz4Block *B = (const Lz4Block *)blocks;
	const Lz4Run *R = (const Lz4Run *)runs;
	emu::launch(emu::dim3{1, 1, 1}, emu::dim3{64, 1, 1}, [=]() { zmt_lz4_par_plan_kernel(R, nrun, nblk, out_bytes, P); });
	emu::launch(emu::dim3{nblk, 1, 1}, emu::dim3{64, 1, 1},
		    [=]() { zmt_lz4_par_measure_kernel(stream, stream_bytes, B, nblk, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_lz4_par_scan_kernel(stream, stream_bytes, B, nblk, R, nrun, out, out_bytes, blk_len, run_len, status, P);
	});
	emu::launch(emu::dim3{nblk, 1, 1}, emu::dim3{64, 1, 1}, [=]() { zmt_lz4_par_exec_kernel(stream, B, nblk, R, out, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{LZ4P_RESOLVE_THREADS, 1, 1}, [=]() {
		zmt_lz4_par_resolve_kernel(R, nrun, nblk, out, out_bytes, blk_len, run_len, status, P);
	});
}

int gpumt_lz4_decompress_blocks_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const gpumt_lz4_block *d_blocks,
				    size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun, void *d_out, size_t out_bytes,
				    uint32_t *d_block_len, uint32_t *d_run_len, uint32_t *d_status, int s)
{
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_stream || !d_blocks || !d_runs || !d_out || !d_block_len || !d_run_len ||
	    !d_status || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	/* (the emulated boundary keeps no variants: the environment alone, read once and validated as gpumt_open does) */
	static int par_on = -1;
	if (par_on < 0) {
		const char *e = getenv("GPUMT_LZ4_RUN_PAR");
		par_on = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				par_on = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_LZ4_RUN_PAR=%s ignored (0 or 1)\n", e);
		}
	}
	emu_lz4_decompress_blocks_par((const u8 *)d_stream, stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out,
				      out_bytes, d_block_len, d_run_len, d_status, par_on);
	return GPUMT_OK;
}

/* seg_on = 0, a table without blocks, or seg_bytes no power of two in 256 .. 4 MiB: the serial kernel */
void emu_lz4_decompress_blocks_seg(const u8 *stream, u64 stream_bytes, const void *blocks, u32 nblk, const void *runs,
				   u32 nrun, u8 *out, u64 out_bytes, u32 *blk_len, u32 *run_len, u32 *status, u32 *block_seg,
				   int seg_on, u32 seg_bytes)
{
	for (u32 b = 0; b < nblk; b++)
		block_seg[b] = 0;
	if (!seg_on || !nblk || seg_bytes < 256 || seg_bytes > (4u << 20) || (seg_bytes & (seg_bytes - 1))) {
		emu_lz4_decompress_blocks(stream, stream_bytes, blocks, nblk, runs, nrun, out, out_bytes, blk_len, run_len, status);
		return;
	}
	const u32 ncut = (u32)(out_bytes / seg_bytes) + nblk;
	std::vector<u16> origin((size_t)out_bytes + 4, 0xA5A5); /* scratch starts as garbage */
	std::vector<u32> owner(nblk, LZ4P_NONE), words((size_t)5 * nblk + 1, 0xA5A5A5A5u), cuts((size_t)2 * ncut, 0xA5A5A5A5u),
		xst((size_t)ncut + nblk, 0xA5A5A5A5u), flag(1, 0);
	Lz4Seg P;
	P.origin = origin.data();
	P.owner = owner.data();
	P.mlen = words.data();
	P.mst = P.mlen + nblk;
	P.pos = P.mst + nblk;
	P.nseg = P.pos + nblk;
	P.cbase = P.nseg + nblk;
	P.cut = cuts.data();
	P.xst = xst.data();
	P.flag = flag.data();
	P.shift = (u32)__builtin_ctz(seg_bytes);
	P.ncut = ncut;
	const Lz4Block *B = (const Lz4Block *)blocks;
	const Lz4Run *R = (const Lz4Run *)runs;
	emu::launch(emu::dim3{1, 1, 1}, emu::dim3{64, 1, 1}, [=]() { zmt_lz4_seg_plan_kernel(B, nblk, R, nrun, out_bytes, P); });
	emu::launch(emu::dim3{nblk, 1, 1}, emu::dim3{64, 1, 1},
		    [=]() { zmt_lz4_seg_measure_kernel(stream, stream_bytes, B, nblk, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_lz4_seg_scan_kernel(stream, stream_bytes, B, nblk, R, nrun, out, out_bytes, blk_len, run_len, status, P);
	});
	emu::launch(emu::dim3{ncut + nblk, 1, 1}, emu::dim3{64, 1, 1}, [=]() { zmt_lz4_seg_exec_kernel(stream, B, nblk, R, out, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{LZ4P_RESOLVE_THREADS, 1, 1}, [=]() {
		zmt_lz4_seg_resolve_kernel(R, nrun, nblk, out, out_bytes, blk_len, run_len, status, block_seg, P);
	});
}

int gpumt_lz4_decompress_blocks_seg(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const gpumt_lz4_block *d_blocks,
				    size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun, void *d_out, size_t out_bytes,
				    uint32_t *d_block_len, uint32_t *d_run_len, uint32_t *d_status, uint32_t *d_block_seg, int s)
{
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_stream || !d_blocks || !d_runs || !d_out || !d_block_len || !d_run_len ||
	    !d_status || !d_block_seg || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	/* (the emulated boundary keeps no variants: the environment alone, read once and validated as gpumt_open does) */
	static int seg_on = -1;
	if (seg_on < 0) {
		const char *e = getenv("GPUMT_LZ4_BLOCK_SEG");
		seg_on = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				seg_on = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_LZ4_BLOCK_SEG=%s ignored (0 or 1)\n", e);
		}
	}
	emu_lz4_decompress_blocks_seg((const u8 *)d_stream, stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out,
				      out_bytes, d_block_len, d_run_len, d_status, d_block_seg, seg_on, 65536u);
	return GPUMT_OK;
}

int gpumt_lz4_pack_runs(gpumt_ctx *h, const void *d_out, size_t out_bytes, const gpumt_lz4_run *d_runs,
			const uint32_t *d_run_len, size_t nrun, void *d_packed, size_t packed_bytes, uint64_t *d_pack_off, int s)
{
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_out || !d_runs || !d_run_len || !d_packed || !d_pack_off || nrun == 0 ||
	    nrun > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if ((const u8 *)d_packed < (const u8 *)d_out + out_bytes && (const u8 *)d_out < (const u8 *)d_packed + packed_bytes)
		return GPUMT_E_ARG;
	emu_lz4_pack_runs((const u8 *)d_out, out_bytes, d_runs, d_run_len, (u32)nrun, (u8 *)d_packed, packed_bytes, d_pack_off);
	return GPUMT_OK;
}

/* the record decoders over the emulator: emu_lz4_decompress_batch (tests/emu/emu_api.cpp) is gpumt_lz4_decompress_batch;
 * emu_lz4_records_kept is the record pass of gpumt_lz4_decompress_batch_par, the same launches with the kernels that take
 * the kept array, the caller's checksum words and no verify pass (variant: 1 = the wave-per-record kernel alone) */
void zmt_xxh32_kernel(const u8 *, const u64 *, const u32 *, u32, u32 *, const u32 *, const u32 *, u32 *);
void zmt_dec_nblk_kernel(const u32 *, u32, u32 *);
void zmt_dec_frames_kept_kernel(const u8 *, const u64 *, const u32 *, u32, const u32 *, const u64 *, u64 *, u32 *, u32 *, u32 *,
				u32 *, u32 *, u32 *, const u32 *);
void zmt_dec_parse4_kernel(const u8 *, u64, const u64 *, const u32 *, const u64 *, u16 *, u32 *, u32 *);
void zmt_dec_copy3_w4_kernel(const u8 *, u64, u32, u32, u8 *, const u64 *, const u32 *, const u64 *, const u64 *, const u32 *,
			     const u32 *, const u32 *, const u16 *, const u32 *, const u32 *, u32 *);
void emu_lz4_decompress_batch(int variant, const u8 *stream, u64 stream_bytes, const u64 *rec_off, const u32 *rec_len,
			      u32 nrec, u8 *out, u64 out_bytes, const u64 *out_off, u32 *out_len, u32 *status);

static void emu_lz4_records_kept(int variant, const u8 *stream, u64 stream_bytes, const u64 *rec_off, const u32 *rec_len,
				 u32 nrec, u8 *out, u64 out_bytes, const u64 *out_off, u32 *out_len, u32 *status,
				 const u32 *kept, u32 *cep, u32 *cvp)
{
	if (variant == 1) {
		emu::launch(emu::dim3{nrec, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
			zmt_lz4_dec_serial_kept(stream, rec_off, rec_len, nrec, out, out_off, out_len, status, cep, cvp, 0xFFFFFFFFu, kept);
		});
		return;
	}
	const size_t nblk_max = out_bytes / 65536 + nrec + 1;
	const size_t ntok_max = stream_bytes / 3 + 128 * nblk_max + 256;
	/* scratch starts as garbage, like device memory */
	std::vector<u32> est(nrec, 0xA5A5A5A5u), rnb(nrec, 0xA5A5A5A5u), rfl(nrec, 0xA5A5A5A5u), bcs(nblk_max, 0x00A5A5A5u),
		bnt(nblk_max, 0xA5A5A5A5u), bol(nblk_max, 0xA5A5A5A5u);
	std::vector<u64> blk0(nrec + 1, 0xA5A5A5A5A5A5A5A5ull), bco(nblk_max, 0x00A5A5A5A5A5A5A5ull);
	std::vector<u16> tok(ntok_max, 0xA5A5);
	u32 *estp = est.data(), *rnbp = rnb.data(), *rflp = rfl.data(), *bcsp = bcs.data(), *bntp = bnt.data(), *bolp = bol.data();
	u64 *blk0p = blk0.data(), *bcop = bco.data();
	u16 *tokp = tok.data();
	emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1}, [=]() { zmt_dec_nblk_kernel(out_len, nrec, estp); });
	emu::launch(emu::dim3{1, 1, 1}, emu::dim3{1024, 1, 1}, [=]() { zmt_scan_kernel(estp, nrec, blk0p); });
	emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1}, [=]() {
		zmt_dec_frames_kept_kernel(stream, rec_off, rec_len, nrec, out_len, blk0p, bcop, bcsp, rnbp, rflp, status, cep, cvp, kept);
	});
	emu::launch(emu::dim3{(u32)((nblk_max + 63) / 64), 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_dec_parse4_kernel(stream, stream_bytes, bcop, bcsp, blk0p + nrec, tokp, bntp, bolp);
	});
	emu::launch(emu::dim3{nrec, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_dec_copy3_w4_kernel(stream, stream_bytes, 0, nrec, out, out_off, out_len, blk0p, bcop, bcsp, rnbp, rflp, tokp, bntp, bolp,
					status);
	});
	emu::launch(emu::dim3{nrec, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_lz4_dec_serial_kept(stream, rec_off, rec_len, nrec, out, out_off, out_len, status, cep, cvp, 100u, kept);
	});
}

/* gpumt_lz4_decompress_batch_par with its knobs as arguments (variant: the record decoders' pipeline, as
 * emu_lz4_decompress_batch; seg_on: the seg route with seg_bytes; cap_mb: 0 = none); stats (may be NULL) receives what the
 * trace line of the real boundary prints: records, par, blocks, slices, fallback */
void emu_lz4_decompress_batch_par(int variant, const u8 *stream, u64 stream_bytes, const u64 *rec_off, const u32 *rec_len,
				  u32 nrec, u8 *out, u64 out_bytes, const u64 *out_off, u32 *out_len, u32 *status, u32 *rec_par,
				  u32 min_blocks, u32 slice_blocks, int par_on, int seg_on, u32 seg_bytes, u32 cap_mb, u32 *stats)
{
	u32 st5[5] = {nrec, 0, 0, 0, 0};
	for (u32 i = 0; rec_par && i < nrec; i++)
		rec_par[i] = 0;
	if (!par_on) {
		emu_lz4_decompress_batch(variant, stream, stream_bytes, rec_off, rec_len, nrec, out, out_bytes, out_off, out_len, status);
		if (stats)
			memcpy(stats, st5, sizeof st5);
		return;
	}
	std::vector<LRec> recv(nrec);
	std::vector<u32> sst(nrec, 0), ce(nrec, 0xA5A5A5A5u), cv(nrec, 0), rfv(nrec, 0xA5A5A5A5u), rrv(nrec, 0xA5A5A5A5u);
	LRec *recs = recv.data();
	u32 *sstp = sst.data(), *cep = ce.data(), *cvp = cv.data(), *rfp = rfv.data(), *rrp = rrv.data();
	const u32 count_seg = seg_on ? seg_bytes : 0;
	emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1}, [=]() {
		zmt_lz4_rec_count_kernel(stream, stream_bytes, rec_off, rec_len, nrec, out_off, out_len, out_bytes, min_blocks,
					 count_seg, recs);
	});
	LRecSlice S;
	/* the scratch the real boundary would ask for: per record, and the largest slice's tables */
	size_t max_blk = 0, max_run = 0, nslices = 0;
	for (size_t at = 0; lrec_next_slice(recs, nrec, at, slice_blocks, &S); at = S.b) {
		max_blk = S.nblk > max_blk ? S.nblk : max_blk;
		max_run = S.nrun > max_run ? S.nrun : max_run;
		nslices++;
	}
	const size_t need = (size_t)nrec * (sizeof(LRec) + 20) + max_blk * (sizeof(Lz4Block) + 8) + max_run * (sizeof(Lz4Run) + 8);
	if (!nslices || (cap_mb && need > ((size_t)cap_mb << 20))) {
		st5[4] = nslices ? 1 : 0;
		emu_lz4_decompress_batch(variant, stream, stream_bytes, rec_off, rec_len, nrec, out, out_bytes, out_off, out_len, status);
		if (stats)
			memcpy(stats, st5, sizeof st5);
		return;
	}
	for (size_t at = 0; lrec_next_slice(recs, nrec, at, slice_blocks, &S); at = S.b) {
		const u32 n = (u32)(S.b - S.a), nblk = S.nblk, nrun = S.nrun;
		std::vector<Lz4Block> blkv(nblk);
		std::vector<Lz4Run> runv(nrun);
		std::vector<u32> blv(nblk, 0xA5A5A5A5u), bsv(nblk, 0xA5A5A5A5u), rlv(nrun, 0xA5A5A5A5u), rsv(nrun, 99u);
		Lz4Block *blk = blkv.data();
		Lz4Run *run = runv.data();
		u32 *rl = rlv.data(), *rs = rsv.data();
		const LRec *sr = recs + S.a;
		u32 *sf = rfp + S.a, *sn = rrp + S.a;
		const u64 in_lo = S.in_lo, out_lo = S.out_lo;
		emu::launch(emu::dim3{1, 1, 1}, emu::dim3{256, 1, 1}, [=]() { zmt_lz4_rec_scan_kernel(sr, n, sf, sn); });
		emu::launch(emu::dim3{(n + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
			    [=]() { zmt_lz4_rec_table_kernel(stream, sr, n, sf, sn, in_lo, out_lo, nblk, nrun, blk, run); });
		if (seg_on)
			emu_lz4_decompress_blocks_seg(stream + S.in_lo, S.in_hi - S.in_lo, blk, nblk, run, nrun, out + S.out_lo,
						      S.out_hi - S.out_lo, blv.data(), rl, rs, bsv.data(), 1, seg_bytes);
		else
			emu_lz4_decompress_blocks_par(stream + S.in_lo, S.in_hi - S.in_lo, blk, nblk, run, nrun, out + S.out_lo,
						      S.out_hi - S.out_lo, blv.data(), rl, rs, 1);
		u32 *ol = out_len + S.a, *rp = rec_par ? rec_par + S.a : nullptr, *ss = sstp + S.a, *e = cep + S.a, *v = cvp + S.a;
		emu::launch(emu::dim3{(n + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
			    [=]() { zmt_lz4_rec_finish_kernel(stream, sr, n, sn, nrun, rl, rs, ol, rp, ss, e, v); });
		st5[1] += nrun;
		st5[2] += nblk;
		st5[3]++;
	}
	/* the record decoders judge everything the block stages did not keep */
	emu_lz4_records_kept(variant, stream, stream_bytes, rec_off, rec_len, nrec, out, out_bytes, out_off, out_len, status, sstp, cep,
			     cvp);
	emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
		    [=]() { zmt_lz4_rec_merge_kernel(sstp, nrec, status, rec_par); });
	emu::launch(emu::dim3{(nrec * 4 + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
		    [=]() { zmt_xxh32_kernel(out, out_off, out_len, nrec, nullptr, cep, cvp, status); });
	if (stats)
		memcpy(stats, st5, sizeof st5);
}

static int emu_lrec_env(const char *name, int lo, int hi, int dflt)
{
	const char *e = getenv(name);
	if (!e || !*e)
		return dflt;
	char *end;
	const long v = strtol(e, &end, 10);
	if (*end || v < lo || v > hi) {
		fprintf(stderr, "gpumt: %s=%s ignored (%d..%d)\n", name, e, lo, hi);
		return dflt;
	}
	return (int)v;
}

int gpumt_lz4_decompress_batch_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				   const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				   const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int s)
{
	static_assert(sizeof(LRec) == 56, "record layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	/* (the environment alone, as the block calls above; read once, by whichever thread comes first: the initialisation of
	 * a function-local static is synchronised) */
	struct Knobs {
		int min_blocks, slice_blocks, seg, trace;
		Knobs()
		{
			const char *e = getenv("GPUMT_TRACE");
			trace = e && *e ? atoi(e) : 0;
			slice_blocks = emu_lrec_env("GPUMT_LZ4_REC_SLICE_BLOCKS", 2, 65536, 4096);
			min_blocks = emu_lrec_env("GPUMT_LZ4_REC_MIN_BLOCKS", 2, 65536, 4096);
			seg = emu_lrec_env("GPUMT_LZ4_REC_SEG", 0, 1, 0);
		}
	};
	static const Knobs knobs;
	u32 st5[5];
	emu_lz4_decompress_batch_par(0, (const u8 *)d_stream, stream_bytes, d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, out_bytes,
				     d_out_off, d_out_len, d_status, d_rec_par, (u32)knobs.min_blocks, (u32)knobs.slice_blocks, 1,
				     knobs.seg, 65536u, 0, st5);
	if (knobs.trace >= 1)
		fprintf(stderr, "[gpumt lz4 rec] records %u par %u blocks %u slices %u fallback %u route %s\n", st5[0], st5[1], st5[2],
			st5[3], st5[4], knobs.seg ? "seg" : "par");
	return GPUMT_OK;
}
}
#endif
