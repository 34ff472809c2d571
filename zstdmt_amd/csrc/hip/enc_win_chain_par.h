/*
 * enc_win_chain_par.h -- the chain plane of the whole-chunk window built in segments (included by zstd_enc.hip behind
 * zstd_enc_win.h; opt-in, gpumt_set_variant "win_chain_par" / GPUMT_WIN_CHAIN_PAR).  zmt_zstd_win_chain_kernel gives a
 * chunk to one wave; here a chunk is cut into segments of S = 1 << seg_log positions (chunk-relative, S >= 4096 and so a
 * multiple of the 64-position step; only a chunk's last segment is partial; none crosses a chunk), and three launches,
 * one after the other on the call's stream, write the same plane word for word.  No wave waits for another inside a kernel.
 *
 *   zmt_win_chain_seg_kernel    persistent waves, one segment at a time, the serial kernel's step (zw_chain_step) with the
 *                               chunk's hlog and the chunk's end, over a head table PER SEGMENT in global scratch (reset
 *                               by the wave; 1 << hlog words at a stride of 1 << hslog).  Afterwards prev[p] = the nearest
 *                               earlier position of the same SEGMENT with p's hash, or ZW_NONE, and heads[seg][h] = the
 *                               last position of the segment with hash h, or ZW_NONE.
 *   zmt_win_chain_carry_kernel  one thread per (chunk, hash), neighbours in h (coalesced), serial over the chunk's
 *                               segments, in place: heads[seg][h] becomes the last position with hash h in segments
 *                               0..seg of the chunk.
 *   zmt_win_chain_patch_kernel  one thread per position; in segments >= 1, a position with a hash whose prev is still
 *                               ZW_NONE takes heads[seg - 1][hash]: the nearest earlier position of the chunk, or ZW_NONE.
 *
 * Segment sg of a slice is segment sg % spc of chunk sg / spc (spc = the segments of a full chunk); the segments a short
 * last chunk does not have are skipped by all three.  A short last chunk uses its own hlog inside the common stride.
 */
#ifndef ZMT_ENC_WIN_CHAIN_PAR_H
#define ZMT_ENC_WIN_CHAIN_PAR_H

extern "C" __global__ void __launch_bounds__(64)
zmt_win_chain_seg_kernel(const u8 *__restrict__ in, u64 n, u32 chunk, u32 seg_log, u32 spc, u32 nseg, u32 hslog,
			 u32 *__restrict__ plane, u32 *__restrict__ heads)
{
	const int lane = wv_lane();
	for (u32 sg = blockIdx.x; sg < nseg; sg += gridDim.x) {
		const u32 rec = sg / spc, s0 = (sg - rec * spc) << seg_log;
		const u64 cstart = (u64)rec * chunk;
		if (cstart >= n)
			continue; /* (an empty input: one record without bytes) */
		const u32 clen = (u32)(n - cstart < chunk ? n - cstart : chunk);
		if (s0 >= clen)
			continue; /* (a short last chunk) */
		const u32 s1 = clen - s0 > (1u << seg_log) ? s0 + (1u << seg_log) : clen;
		u32 *const head = heads + ((u64)sg << hslog);
		const u32 hlog = zw_hlog(clen);
		for (u32 i = (u32)lane; i < (1u << hlog); i += 64)
			head[i] = ZW_NONE;
		wave_mem_fence();
		wv_sync();
		for (u32 p0 = s0; p0 < s1; p0 += 64)
			zw_chain_step(in + cstart, clen, hlog, p0, lane, plane + cstart, head);
	}
}

/* grid: nrec << hslog threads in blocks of 256 (hslog >= ZW_HLOG_MIN: a block stays inside one chunk) */
extern "C" __global__ void __launch_bounds__(256)
zmt_win_chain_carry_kernel(u64 n, u32 chunk, u32 seg_log, u32 spc, u32 nrec, u32 hslog, u32 *__restrict__ heads)
{
	const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
	const u32 rec = (u32)(t >> hslog), h = (u32)t & ((1u << hslog) - 1u);
	const u64 cstart = (u64)rec * chunk;
	if (rec >= nrec || cstart >= n)
		return;
	const u32 clen = (u32)(n - cstart < chunk ? n - cstart : chunk);
	if (h >= (1u << zw_hlog(clen)))
		return;
	const u32 segs = (u32)(((u64)clen + (1u << seg_log) - 1) >> seg_log);
	u32 *w = heads + ((u64)rec * spc << hslog) + h;
	u32 last = ZW_NONE;
	for (u32 k = 0; k < segs; k++, w += (size_t)1 << hslog) {
		const u32 e = *w;
		if (e != ZW_NONE)
			last = e;
		else if (last != ZW_NONE)
			*w = last;
	}
}

/* grid: one thread per input byte of the slice (n <= 2^30) in blocks of 256 */
extern "C" __global__ void __launch_bounds__(256)
zmt_win_chain_patch_kernel(const u8 *__restrict__ in, u64 n, u32 chunk, u32 seg_log, u32 spc, u32 hslog,
			   u32 *__restrict__ plane, const u32 *__restrict__ heads)
{
	const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
	if (g >= n)
		return;
	const u32 rec = (u32)g / chunk, p = (u32)g - rec * chunk, k = p >> seg_log;
	const u64 cstart = (u64)rec * chunk;
	const u32 clen = (u32)(n - cstart < chunk ? n - cstart : chunk);
	if (k == 0 || p + ZE_HBYTES > clen || plane[g] != ZW_NONE)
		return;
	/* (reads up to 2 bytes behind the chunk: the next chunk's, or the input's slack) */
	const u32 h = ze_hash<ZE_HBYTES, ZW_HLOG_MAX>(ld64u(in + g)) >> (ZW_HLOG_MAX - zw_hlog(clen));
	plane[g] = heads[(((u64)rec * spc + k - 1) << hslog) + h];
}

#endif
