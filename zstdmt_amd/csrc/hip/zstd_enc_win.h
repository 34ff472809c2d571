/*
 * zstd_enc_win.h -- whole-chunk match window for the zstd encoder (included by zstd_enc.hip; opt-in,
 * gpumt_zstd_compress_batch_win): hash chains over the chunk instead of one probe into an LDS table.
 *
 *   zmt_zstd_win_chain_kernel  persistent waves, one chunk at a time, 64 positions per step in order: every
 *                              position is hashed over ZE_HBYTES bytes; a head table of u32 positions in
 *                              global scratch (one per resident wave, reset per chunk) says where a hash
 *                              occurred last; the kernel writes the CHAIN PLANE, one u32 per input byte:
 *                              prev[p] = the nearest earlier position of the same chunk with p's hash, or
 *                              ZW_NONE.  The plane is a function of the chunk's bytes alone.
 *   ze_win_find                the match finder of zmt_zstd_enc_win_kernel (zstd_enc_body<..., WIN = true>):
 *                              lane p walks prev from prev[p] for at most `depth` candidates, all lanes issue
 *                              candidate k's loads together (64 independent chains per wave, no LDS table),
 *                              and keeps the best by zstd's own rule, 4 * length - log2(offset + 1), ties to
 *                              the nearer.  A candidate may lie in any earlier block of the chunk; the rest of
 *                              the block stage (parse, literals, Huffman, FSE, sub-blocks) is the body's.
 *
 * Positions of the plane are relative to the chunk.  Inside the body a candidate stays relative to the block, as
 * the table encoders have it, and is negative (as a wrapped u32) when it lies in an earlier block; ZW_FAR stands
 * for "no candidate" there (no distance reaches 2^31).
 */
#ifndef ZMT_ZSTD_ENC_WIN_H
#define ZMT_ZSTD_ENC_WIN_H

#include "enc_win_common.h" /* ZW_NONE, ZW_FAR, ZW_HLOG_*, ze_at: shared with the brotli encoder's window */
#define ZW_MAXDIST (1u << 27)    /* offset codes <= 27: what the predefined offset table covers */

static __device__ __forceinline__ u32 zw_hlog(u32 clen)
{
	const int l = 31 - __builtin_clz(clen | 1u) - 3;
	return (u32)(l > ZW_HLOG_MAX ? ZW_HLOG_MAX : l < ZW_HLOG_MIN ? ZW_HLOG_MIN : l);
}

/* One step of the chain build: the 64 positions from p0 (a multiple of 64 inside the chunk of clen bytes at base) are hashed
 * and linked in position order through `head`, 1 << hlog words.  Shared by the serial kernel below and the segment kernel
 * of enc_win_chain_par.h, so both write the same words wherever their head tables agree. */
static __device__ __forceinline__ void zw_chain_step(const u8 *__restrict__ base, u32 clen, u32 hlog, u32 p0, int lane,
						     u32 *__restrict__ prev, u32 *__restrict__ head)
{
	const u32 p = p0 + (u32)lane;
	/* (reads up to 7 bytes behind the chunk: the next chunk's, or the input's slack, include/gpumt.h) */
	const u64 v = ld64u(base + (p < clen ? p : clen - 1));
	const bool ok = p + ZE_HBYTES <= clen; /* the last ZE_HBYTES - 1 positions have no hash */
	const u32 h = ze_hash<ZE_HBYTES, ZW_HLOG_MAX>(v) >> (ZW_HLOG_MAX - hlog);
	const u32 e = head[ok ? h : 0u];
	/* the lanes of this step with my hash: one ballot per hash bit.  A lane chains to the nearest such lane
	 * below it and only the first of them to the table's entry; the highest writes the head -- so the plane
	 * does not depend on the order the memory serves the lanes in */
	u64 same = wv_ballot(ok);
	for (u32 b = 0; b < hlog; b++) {
		const bool bit = (h >> b) & 1u;
		const u64 m = wv_ballot(bit);
		same &= bit ? m : ~m;
	}
	const u64 lower = same & ((1ull << lane) - 1ull), higher = (same >> lane) >> 1;
	if (p < clen)
		prev[p] = !ok ? ZW_NONE : lower ? p0 + 63u - (u32)__builtin_clzll(lower) : e;
	if (ok && !higher)
		head[h] = p;
	wave_mem_fence(); /* the next step reads what this one wrote */
	wv_sync();
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_win_chain_kernel(const u8 *__restrict__ in, u64 n, u32 chunk, u32 nrec, u32 *__restrict__ plane,
			  u32 *__restrict__ heads)
{
	const int lane = wv_lane();
	u32 *const head = heads + ((u64)blockIdx.x << ZW_HLOG_MAX);
	for (u32 rec = blockIdx.x; rec < nrec; rec += gridDim.x) {
		const u64 cstart = (u64)rec * chunk;
		if (cstart >= n)
			continue; /* (an empty input: one record without bytes) */
		const u32 clen = (u32)(n - cstart < chunk ? n - cstart : chunk);
		const u8 *const base = in + cstart;
		u32 *const prev = plane + cstart;
		const u32 hlog = zw_hlog(clen);
		for (u32 i = (u32)lane; i < (1u << hlog); i += 64)
			head[i] = ZW_NONE;
		wave_mem_fence();
		wv_sync();
		for (u32 p0 = 0; p0 < clen; p0 += 64)
			zw_chain_step(base, clen, hlog, p0, lane, prev, head);
	}
}

/* The best candidate of position p (block-relative, `ok` = it has one at all: inside the block with room for the shortest
 * match), as a block-relative position, or ZW_FAR.  cprev / cbase = the chunk's plane and bytes; v, d8, d16 = the input's bytes
 * 0..7, 8..15, 16..19.  Wave-uniform control flow: every lane walks while any lane has a candidate left. */
template <u32 MM>
static __device__ __forceinline__ u32 ze_win_find(const u8 *__restrict__ cbase, const u32 *__restrict__ cprev, u32 bstart,
						   u32 bsize, u32 p, bool ok, u64 v, u64 d8, u32 d16, u32 depth)
{
	const u32 pa = bstart + p; /* position in the chunk */
	/* a candidate's distance is at most min(position in the chunk, 2^27); the compare window of the body starts 4
	 * bytes in front of a candidate, so the chunk's first four positions are none (as a block's are none for the
	 * table encoders).  ZW_NONE is pa + 1 away: the end of a chain fails the same test */
	const u32 reach = pa >= 4u ? pa - 4u : 0u, maxd = reach < ZW_MAXDIST ? reach : ZW_MAXDIST;
	const u32 room = ok ? bsize - p : 0u; /* a match ends with its block */
	u32 c = cprev[ok ? pa : 0u];
	u32 best = ZW_FAR;
	int bscore = 0;
	for (u32 k = 0; k < depth; k++) {
		const u32 dist = pa - c;
		const bool live = ok && dist - 1u < maxd;
		if (!wv_any(live))
			break;
		const u32 cs = live ? c : 0u;
		const u64 a = ld64u(cbase + cs);
		const u32 nxt = cprev[cs];
		const u64 x0 = a ^ v;
		u32 m = x0 ? (u32)__builtin_ctzll(x0) >> 3 : 8u;
		if (live && m == 8u) { /* the existing 8-byte compares, the next 12 bytes only where 8 agree (no cross-lane work inside) */
			const u64 x1 = ld64u(cbase + cs + 8) ^ d8;
			const u32 x2 = ld32u(cbase + cs + 16) ^ d16;
			m = x1 ? 8u + ((u32)__builtin_ctzll(x1) >> 3) : x2 ? 16u + ((u32)__builtin_ctz(x2) >> 3) : ZE_FWD;
		}
		const bool full = m == ZE_FWD; /* measured to the end of what is compared: nothing further on can beat it */
		m = m < room ? m : room;
		const int score = 4 * (int)m - (31 - __builtin_clz(dist + 1u));
		if (live && m >= MM && score > bscore) { /* (strictly: ties stay with the nearer) */
			bscore = score;
			best = c - bstart;
		}
		c = (live && !full) ? nxt : ZW_NONE;
	}
	return best;
}

#endif
