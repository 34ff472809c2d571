/*
 * enc_win_common.h -- what the whole-chunk-window encoders share (zstd_enc_win.h, brotli_enc_win.h): the constants of the
 * CHAIN PLANE that zmt_zstd_win_chain_kernel (zstd_enc_win.h, once in the library) writes -- per input byte the nearest
 * earlier position of the same chunk whose next 6 bytes hash alike -- and the block-relative addressing of a candidate
 * that may lie in an earlier block.  The plane is a function of the chunk's bytes alone, so every codec walks the same one.
 */
#ifndef ZMT_ENC_WIN_COMMON_H
#define ZMT_ENC_WIN_COMMON_H

#define ZW_NONE 0xFFFFFFFFu      /* plane: no earlier position with this hash */
#define ZW_FAR 0x80000000u       /* body: "no candidate" among block-relative positions that wrap negative */
#define ZW_HLOG_MAX 17           /* head table: min(17, log2(chunk) - 3) bits, at least ZW_HLOG_MIN */
#define ZW_HLOG_MIN 12
#define ZW_HEAD_BYTES (4u << ZW_HLOG_MAX) /* per resident wave of the chain kernel */

/* base + a block-relative position that may be negative (WIN) */
template <bool WIN> static __device__ __forceinline__ const u8 *ze_at(const u8 *base, u32 rel)
{
	return WIN ? base + (ptrdiff_t)(int)rel : base + rel;
}

#endif
