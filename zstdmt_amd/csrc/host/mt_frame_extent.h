/*
 * mt_frame_extent.h -- frame splitters: where the LZ4 / zstd frame at p ends and how many bytes it can decode
 * to, found by walking its block headers on the host (zstd-mt records whose frame states no content size,
 * d12_out_size in zstdmt_engine.c; the plain-stream paths walk block by block themselves, mt_lz4_plain.inc and
 * mt_zstd_plain.inc).  Pure functions over bytes: nothing of the device boundary is needed here
 * (tests/host/extent_harness.c runs them on the CPU).
 */
#ifndef ZMT_MT_FRAME_EXTENT_H
#define ZMT_MT_FRAME_EXTENT_H

#include <stddef.h>
#include <stdint.h>

#include "mt_le.h"

/* Length of the LZ4 frame at p (n bytes are there), or 0 = the frame is not complete yet (more input may
 * complete it), or EXTENT_INVALID = these bytes cannot become a frame however much follows (descriptor or
 * block size out of the format): the incremental reader stops at once instead of buffering the rest of a
 * damaged stream until its end. */
#define EXTENT_INVALID ((size_t)-1)
static inline size_t lz4_frame_extent(const uint8_t *p, size_t n, uint64_t *bound, int *supported)
{
	if (n < 7)
		return 0;
	const unsigned flg = p[4], bd = p[5];
	const unsigned bsid = (bd >> 4) & 7;
	const int has_csize = (flg >> 3) & 1, has_dict = flg & 1, bchk = (flg >> 4) & 1, cchk = (flg >> 2) & 1;
	size_t hp = 6 + (has_csize ? 8 : 0) + (has_dict ? 4 : 0) + 1;
	uint64_t sum = 0, blkmax;
	if ((flg >> 6) != 1 || (flg & 2) || (bd & 0x8F) || bsid < 4)
		return EXTENT_INVALID; /* version, reserved bits, block size id (what LZ4F_decompress rejects first) */
	if (n < hp)
		return 0;
	blkmax = 1ull << (8 + 2 * bsid); /* 4 -> 64 KiB ... 7 -> 4 MiB */
	*supported = 1; /* block checksums are verified and a dictionary id skipped by the frame-serial kernel */
	for (;;) {
		uint32_t bh, bsz;
		if (n - hp < 4)
			return 0;
		bh = rd32(p + hp);
		hp += 4;
		if (bh == 0)
			break;
		bsz = bh & 0x7FFFFFFFu;
		if (bsz > blkmax)
			return EXTENT_INVALID;
		if (n - hp < bsz + (bchk ? 4u : 0u))
			return 0;
		hp += bsz + (bchk ? 4u : 0u);
		sum += (bh & 0x80000000u) ? bsz : blkmax;
	}
	if (cchk) {
		if (n - hp < 4)
			return 0;
		hp += 4;
	}
	*bound = has_csize ? rd64(p + 6) : sum;
	return hp;
}

/* one zstd frame at p[0..n): total length and output bound; 0 = not complete yet, EXTENT_INVALID = cannot become a
 * frame (reserved bit, reserved block type, block larger than the format allows) */
static inline size_t zstd_frame_extent(const uint8_t *p, size_t n, uint64_t *bound, int *sized)
{
	if (n < 6)
		return 0;
	const unsigned fhd = p[4], fcs = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3, chk = (fhd >> 2) & 1;
	const unsigned did_len = did == 3 ? 4 : did, fcs_len = fcs == 0 ? single : 1u << fcs;
	size_t hp = 5;
	uint64_t window = 0, content = 0, sum = 0;
	if (fhd & 8)
		return EXTENT_INVALID; /* reserved bit */
	if (n < 5 + (1 - single) + did_len + fcs_len)
		return 0;
	if (!single) {
		const unsigned wd = p[hp++];
		const uint64_t base = 1ull << (10 + (wd >> 3));
		window = base + (base >> 3) * (wd & 7);
	}
	hp += did_len;
	for (unsigned k = 0; k < fcs_len; k++)
		content |= (uint64_t)p[hp + k] << (8 * k);
	if (fcs == 1)
		content += 256;
	hp += fcs_len;
	if (single)
		window = content;
	const uint64_t block_max = window < 131072 ? window : 131072;
	for (;;) {
		if (n - hp < 3)
			return 0;
		const uint32_t bh = (uint32_t)p[hp] | (uint32_t)p[hp + 1] << 8 | (uint32_t)p[hp + 2] << 16;
		const uint32_t last = bh & 1, type = (bh >> 1) & 3, bsize = bh >> 3;
		hp += 3;
		if (type == 3 || (type != 1 && bsize > 131072u))
			return EXTENT_INVALID; /* reserved block type; Block_Maximum_Size is 128 KiB at most (RFC 8878 3.1.1.2.4) */
		if (type == 1) { /* RLE: one byte regenerates bsize */
			if (n - hp < 1)
				return 0;
			hp += 1;
			sum += bsize;
		} else {
			if (n - hp < bsize)
				return 0;
			hp += bsize;
			sum += type == 0 ? bsize : block_max;
		}
		if (last)
			break;
	}
	if (chk) {
		if (n - hp < 4)
			return 0;
		hp += 4;
	}
	*sized = fcs_len != 0;
	*bound = fcs_len ? content : sum;
	return hp;
}

#endif
