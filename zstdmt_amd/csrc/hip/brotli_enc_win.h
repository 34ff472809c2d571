/*
 * brotli_enc_win.h -- whole-chunk match window for the brotli encoder (included by brotli_enc.hip; opt-in,
 * gpumt_brotli_compress_batch_win, qualities 9-11): hash chains over the chunk instead of one probe into an LDS table.
 *
 *   the chain plane   zmt_zstd_win_chain_kernel's (zstd_enc_win.h; the kernel exists once in the library): prev[p] = the
 *                     nearest earlier position of the same chunk whose next 6 bytes hash alike, or ZW_NONE -- the bytes
 *                     be_hash hashes, by the zstd encoder's function, so a false twin costs one compare.
 *   be_win_find       the match finder of zmt_brotli_enc_win_kernel (brotli_enc_body<..., WIN = true>): lane p walks prev
 *                     from prev[p] for at most `depth` candidates, all lanes issue candidate k's loads together, measures
 *                     each on the 24 bytes the body compares and keeps the best by 4 * length - log2(distance + 1), ties
 *                     to the nearer.  A candidate may lie in any earlier block of the chunk; the rest of the block stage
 *                     (parse, histograms, prefix codes, commands, the uncompressed fall-back) is the body's.
 *
 * Stream rules (RFC 7932): a distance beyond min(bytes written so far, (1 << WBITS) - 16) would be read as a reference
 * into the static dictionary, so a candidate's distance is at most min(position in the chunk, (1 << WBITS) - 16) with
 * be_win_wbits(chunk length) the WBITS block 0 writes; chunks above 16 MiB rely on the cap alone.
 */
#ifndef ZMT_BROTLI_ENC_WIN_H
#define ZMT_BROTLI_ENC_WIN_H

#include "enc_win_common.h"

#define BW_CMP 24u /* bytes of a match the body's Cmp measures; longer ones by the whole wave */

/* the smallest WBITS in 18..24 whose window, (1 << WBITS) - 16, holds the chunk's largest distance, clen - 1; else 24 */
static __device__ __forceinline__ u32 be_win_wbits(u32 clen)
{
	u32 wb = 18;
	while (wb < 24 && (1u << wb) - 16u < clen - 1u)
		wb++;
	return wb;
}

/* The best candidate of position p (block-relative, `ok` = it has one at all: inside the block with room for the shortest
 * match) as a block-relative position that wraps below zero for an earlier block, or ZW_FAR.  cprev / cbase = the chunk's
 * plane and bytes; v, d8, d16 = the input's bytes 0..7, 8..15, 16..23; window = (1 << WBITS) - 16.  Wave-uniform control
 * flow: every lane walks while any lane has a candidate left. */
template <u32 MM>
static __device__ __forceinline__ u32 be_win_find(const u8 *__restrict__ cbase, const u32 *__restrict__ cprev, u32 bstart,
						   u32 bsize, u32 p, bool ok, u64 v, u64 d8, u64 d16, u32 depth, u32 window)
{
	const u32 pa = bstart + p; /* position in the chunk */
	/* the end of a chain, ZW_NONE, is pa + 1 away and fails the same test as a candidate out of reach */
	const u32 maxd = pa < window ? pa : window;
	const u32 room = ok ? bsize - p : 0u; /* a match ends with its block: a copy may not run past MLEN */
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
		if (live && m == 8u) { /* the next 16 bytes only where 8 agree (no cross-lane work inside) */
			const u64 x1 = ld64u(cbase + cs + 8) ^ d8, x2 = ld64u(cbase + cs + 16) ^ d16;
			m = x1 ? 8u + ((u32)__builtin_ctzll(x1) >> 3) : x2 ? 16u + ((u32)__builtin_ctzll(x2) >> 3) : BW_CMP;
		}
		const bool full = m == BW_CMP; /* agrees over everything compared: nothing further on is looked at */
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
