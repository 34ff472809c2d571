/*
 * brotlimt_engine.c -- the host side of brotli-mt on MI355X: BROTLIMT_* (include/brotli-mt.h) over
 * gpumt_*: mt16_engine.inc with brotli's constants (reference lib/brotli-mt_compress.c,
 * lib/brotli-mt_decompress.c).
 */
#include "mt_host.h"
#include "brotli-mt.h"

#define MTP(x) BROTLIMT_##x
#define MT_CODEC "brotli"
#define MT_LEVEL_OK(level) ((level) >= BROTLIMT_LEVEL_MIN && (level) <= BROTLIMT_LEVEL_MAX)
#define MT_DEFAULT_CHUNK(level) (1024 * 1024 * ((level) ? (level) : 1)) /* lib/brotli-mt_compress.c:105-109 */
#define MT_SLOT_STRIDE(chunk) gpumt_zstd_slot_stride(chunk)
/* the quality reaches the encoder as the reference hands it to BrotliEncoderCompress (lib/brotli-mt_compress.c:269-272) */
/* GPUMT_BROTLI_WIN=1 (exactly that) hands qualities 9-11 to the whole-chunk-window encoder instead,
 * gpumt_brotli_compress_batch_win: same slots, same records, smaller streams; unset or anything else, and below quality 9,
 * the call is the one above, byte for byte.  The variable is read per batch (the launching thread alone reads it).  A weak
 * reference, as in zstdmt_engine.c: a stand-in for the device boundary that lacks the call leaves the engine on the table
 * encoder */
extern __typeof__(gpumt_brotli_compress_batch_win) gpumt_brotli_compress_batch_win __attribute__((weak));
static int brotli_compress_batch(gpumt_ctx *g, const void *d_in, size_t n, size_t chunk, void *d_slots, size_t stride,
				 uint32_t *d_len, int level, int stream)
{
	const char *e = level >= 9 && gpumt_brotli_compress_batch_win ? getenv("GPUMT_BROTLI_WIN") : NULL;
	if (e && e[0] == '1' && !e[1])
		return gpumt_brotli_compress_batch_win(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
	return gpumt_brotli_compress_batch_level(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
}
#define MT_COMPRESS_BATCH brotli_compress_batch
#define MT_DECOMPRESS_BATCH gpumt_brotli_decompress_batch
#define MT_CAP_FROM_PREAMBLE 0 /* capacity = hint << 16, lib/brotli-mt_decompress.c:236-239 */

#include "mt16_engine.inc"
