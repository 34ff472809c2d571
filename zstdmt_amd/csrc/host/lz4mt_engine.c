/*
 * lz4mt_engine.c -- the host side of lz4-mt on MI355X: LZ4MT_* (include/lz4-mt.h) over gpumt_*.
 *
 * Replaces the pthread worker pool of the reference (lib/lz4-mt_compress.c:207-353,
 * lib/lz4-mt_decompress.c:165-567): instead of T threads each pulling one chunk through the codec,
 * one host thread moves *batches* of chunks through a three-stage device pipeline
 *
 *        fn_read -> pinned in[s]  --H2D (stream 1)-->  kernels (stream 0)  --D2H (stream 2)-->
 *        pinned out[s] -> fn_write
 *
 * over the four slots of mt_pipe.h (up to three batches on the device, decompress on per-slot
 * kernel streams, while another is read into or written out).  Callback-visible behaviour follows the reference: compress issues one fn_read of
 * exactly `inputsize` bytes per chunk and one fn_write per record, in input order; decompress
 * reads 4, then 8|12 header bytes and the payload per record, and writes one chunk per call.
 * The compress half is mt_compress.inc, the record pipeline is mt_records12.inc (both shared with zstdmt_engine.c), the
 * plain .lz4 path (block-parallel, frames of any size) is mt_lz4_plain.inc; this file holds what is lz4-mt's own: the error strings, the parameters and hooks of the two
 * texts and the 4-byte sniff of LZ4MT_decompressDCtx.
 * This file is plain C and never includes a HIP header.
 */
#include "mt_host.h"
#include "mt_pipe.h"
#include "lz4-mt.h"

size_t lz4mt_errcode;

/* ------------------------------------------------------------------ errors (lz4-mt_common.c) */
unsigned LZ4MT_isError(size_t code)
{
	return code > ERROR(maxCode);
}

const char *LZ4MT_getErrorString(size_t code)
{
	static const char *const codec[] = {
		"", "device: malformed record header", "device: bad LZ4 frame header",
		"device: malformed LZ4 block", "device: content size mismatch",
		"device: content checksum mismatch", "device: trailing bytes after frame",
		"device: unsupported LZ4 frame feature",
	};
	size_t idx = (size_t)0 - code;
	/* like the reference, a pending codec-level error takes precedence */
	if (lz4mt_errcode >= 1 && lz4mt_errcode <= 7 && idx == LZ4MT_error_compression_library)
		return codec[lz4mt_errcode];
	if (idx < LZ4MT_error_canceled)
		return mt_error_name(idx);
	return "Unspecified lz4mt error code"; /* canceled has no text in the reference either */
}

/* ------------------------------------------------------------------ compression: mt_compress.inc */
#define MTP(x) LZ4MT_##x
#define LZ4MT_ERROR(name) ERROR(name)
#define MT_CODEC "lz4" /* "lz4mt compress" / "lz4mt decompress" at GPUMT_TRACE >= 2 */
#define MT_LEVEL_OK(level) ((level) >= LZ4MT_LEVEL_MIN && (level) <= LZ4MT_LEVEL_MAX)
#define MT_DEFAULT_CHUNK(level) ((void)(level), 1024 * 1024 * 4) /* lz4-mt_compress.c:111-114 */
#define MT_SLOT_STRIDE(chunk) gpumt_lz4_slot_stride(chunk)
#define MT_COMPRESS_BATCH gpumt_lz4_compress_batch_level
/* (twice the chunk: the LZ4 encoder is one wave per chunk at ~20 MB/s -- 512 chunks per batch, 3 batches in flight, is
 * where the device comes near the reader: 12.3 -> 16.8 GB/s at 1 MiB chunks; the other codecs' encoders put several waves
 * on a chunk, and the decompress leg lost 2 GB/s to the coarser pipeline with the same rule) */
#define MT_BATCH_UNIT(chunk) (2 * (chunk))
#define MT_C_DEVICE_ERROR compression_library
#define MT_C_NULL_CTX compressionParameter_unsupported
#define MT_C_NULL_GET 0
/* (a level the device has no encoder for cannot happen for a context createCCtx accepted.)  The reference keeps its
 * counters across calls; so do we */
#define MT_COMPRESS_ENTER(ctx) (gpumt_lz4_level_supported((ctx)->level) ? 0 : ERROR(compressionParameter_unsupported))

#include "mt_compress.inc"

/* ------------------------------------------------------------------ decompression: mt_records12.inc */
#define MT_ERRCODE lz4mt_errcode
#define MT_D_DEFAULT_INPUTSIZE (1024 + 1024 * 4) /* sic, lz4-mt_decompress.c:115 */
#define MT_D12_CHECK_SIZE_FIELD 1
#define MT_D12_STATUS_PRESET 0
/* GPUMT_LZ4_REC_PAR=1 (exactly that) hands the batch to gpumt_lz4_decompress_batch_par, which decodes the records of
 * several linked blocks block-parallel: same records, statuses, sizes and bytes; unset or anything else, the call is the
 * one below, byte for byte.  Read per batch by the launching thread; a weak reference, as in zstdmt_engine.c */
extern __typeof__(gpumt_lz4_decompress_batch_par) gpumt_lz4_decompress_batch_par __attribute__((weak));
static int lz4_decompress_batch(gpumt_ctx *g, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, int stream)
{
	const char *e = gpumt_lz4_decompress_batch_par ? getenv("GPUMT_LZ4_REC_PAR") : NULL;
	if (e && e[0] == '1' && !e[1])
		return gpumt_lz4_decompress_batch_par(g, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes,
						      d_out_off, d_out_len, d_status, NULL, stream);
	return gpumt_lz4_decompress_batch(g, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					  d_out_len, d_status, stream);
}
#define MT_DECOMPRESS_BATCH lz4_decompress_batch
#define MT_FRAME_MAGIC LZ4FMT_MAGICNUMBER
#define MT_PLAIN_REQUEST(ctx) ((size_t)(ctx)->inputsize) /* inputsize requests, lz4-mt_decompress.c:462-476 */
#define MT_PLAIN_PIECE(ctx) ((ctx)->inputsize < 65536 ? (size_t)65536 : (size_t)(ctx)->inputsize)
#define MT_PLAIN_ENTER(ctx, nfirst) ((ctx)->insize = (nfirst), (ctx)->outsize = 0)
#define MT_PLAIN_COUNT_FAILED_WRITE 1

/* output size = LE64 at payload+6 (lz4-mt_decompress.c:333-334); frames that carry no
 * content size (only the empty frame is written that way) decode to nothing */
static size_t d12_out_size(const uint8_t *frame, uint32_t csize, uint64_t *osz, int *unsized)
{
	(void)unsized;
	*osz = csize >= 15 && (frame[4] & 0x08) ? rd64(frame + 6) : 0;
	return *osz > 0xFFFFFFFFull ? ERROR(data_error) : 0;
}

/* pt_decompress: LZ4F error -> compression_library (code kept in the global),
 * frame not consumed exactly -> frame_decompress (lz4-mt_decompress.c:353-362) */
static size_t d12_status_error(uint32_t st)
{
	if (st == GPUMT_ST_BAD_RECORD)
		return ERROR(data_error);
	if (st == GPUMT_ST_TRAILING)
		return ERROR(frame_decompress);
	lz4mt_errcode = st;
	return ERROR(compression_library);
}

/* plain .lz4 streams (typically 4 MiB blocks and no content size) are decoded block by block, mt_lz4_plain.inc */
static size_t plain_bad_frame(void) { return ERROR(compression_library); }

#include "mt_records12.inc"
#include "mt_lz4_plain.inc"

size_t LZ4MT_decompressDCtx(LZ4MT_DCtx *ctx, LZ4MT_RdWr_t *rdwr)
{
	uint8_t magic[4];
	LZ4MT_Buffer b;
	int rv;

	if (!ctx)
		return ERROR(compressionParameter_unsupported); /* lz4-mt_decompress.c:493-494 */
	/* sniff: 4 bytes (lz4-mt_decompress.c:503-520), on the calling thread */
	b.buf = magic;
	b.size = 4;
	b.allocated = 4;
	rv = rdwr->fn_read(rdwr->arg_read, &b);
	if (rv != 0)
		return mt_error(rv);
	if (b.size != 4)
		return ERROR(data_error);
	if (rd32(magic) != LZ4FMT_MAGIC_SKIPPABLE) {
		if (rd32(magic) != LZ4FMT_MAGICNUMBER)
			return ERROR(data_error);
		/* plain .lz4 stream: the reference decodes it single-threaded (st_decompress, :391-483) */
		return lz4_plain_decompress(ctx, rdwr, magic, 4);
	}
	ctx->have_hdr = 0;
	ctx->first_hdr = 1;
	return d12_run(ctx, rdwr);
}
