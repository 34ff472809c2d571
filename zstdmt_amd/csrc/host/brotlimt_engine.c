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
/* GPUMT_BROTLI_INDEX=1 (exactly that): the table encoders' records carry the span index of gpumt_brotli_compress_batch_index
 * -- every decoder skips it, gpumt_brotli_decompress_batch_par cuts the record by it.  The window encoder, where it applies,
 * wins: its blocks are not self-contained and it writes no index.
 * GPUMT_BROTLI_REC_PAR=1 (exactly that): records are decoded by gpumt_brotli_decompress_batch_par, whose results are
 * gpumt_brotli_decompress_batch's for every batch (GPUMT_BROTLI_REC_MIN_SPANS: read by the device layer when the handle
 * opens).  Both are read per batch and weak like the window call */
extern __typeof__(gpumt_brotli_compress_batch_index) gpumt_brotli_compress_batch_index __attribute__((weak));
extern __typeof__(gpumt_brotli_decompress_batch_par) gpumt_brotli_decompress_batch_par __attribute__((weak));
static int env_is_1(const char *name)
{
	const char *e = getenv(name);
	return e && e[0] == '1' && !e[1];
}
static int brotli_compress_batch(gpumt_ctx *g, const void *d_in, size_t n, size_t chunk, void *d_slots, size_t stride,
				 uint32_t *d_len, int level, int stream)
{
	if (level >= 9 && gpumt_brotli_compress_batch_win && env_is_1("GPUMT_BROTLI_WIN"))
		return gpumt_brotli_compress_batch_win(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
	if (gpumt_brotli_compress_batch_index && env_is_1("GPUMT_BROTLI_INDEX"))
		return gpumt_brotli_compress_batch_index(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
	return gpumt_brotli_compress_batch_level(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
}
static int brotli_decompress_batch(gpumt_ctx *g, const void *d_stream, const uint64_t *d_rec_off, const uint32_t *d_rec_len,
				   size_t nrec, void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
				   uint32_t *d_out_len, uint32_t *d_status, int stream)
{
	if (gpumt_brotli_decompress_batch_par && env_is_1("GPUMT_BROTLI_REC_PAR"))
		return gpumt_brotli_decompress_batch_par(g, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap,
							 d_out_len, d_status, NULL, stream);
	return gpumt_brotli_decompress_batch(g, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len,
					     d_status, stream);
}
#define MT_COMPRESS_BATCH brotli_compress_batch
#define MT_DECOMPRESS_BATCH brotli_decompress_batch
#define MT_CAP_FROM_PREAMBLE 0 /* capacity = hint << 16, lib/brotli-mt_decompress.c:236-239 */

#include "mt16_engine.inc"
