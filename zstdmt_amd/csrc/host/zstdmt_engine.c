/*
 * zstdmt_engine.c -- the host side of zstd-mt on MI355X: ZSTDCB_* (include/zstd-mt.h) over gpumt_*.
 *
 * Same pipeline as lz4mt_engine.c (batches of records through H2D / kernels / D2H on three
 * streams, four slots: mt_pipe.h), following the callback-visible behaviour of the reference
 * (lib/zstd-mt_compress.c:208-392, lib/zstd-mt_decompress.c:209-549,693-843):
 *   compress   one fn_read of exactly `inputsize` per chunk, one fn_write per record, in order;
 *              counters are reset per call (:337-341); empty input still yields one frame (:264);
 *   decompress a 16-byte sniff, then csize-4 bytes for the first record, then 12 + csize bytes per
 *              record (:221-353); one fn_write per frame in order.
 * Stream layouts accepted by decompress: the one the compressor writes ("pzstd style": skippable
 * frame first, :251-284) and the old "zstdmt style" (a 9-byte empty zstd frame in front, :225-249).
 * Plain .zst streams (the reference's single-threaded path) are walked block by block on the
 * host and decoded run by run, frames of any size (plain_decompress, mt_zstd_plain.inc).
 * The compress half is mt_compress.inc, the record pipeline is mt_records12.inc (both shared
 * with lz4mt_engine.c); this file holds what is zstd-mt's own: the error strings, the parameters and hooks of the two
 * texts, the content size of a frame and the 16-byte sniff of ZSTDCB_decompressDCtx.
 * Plain C, no HIP header.
 */
#include "mt_host.h"
#include "mt_pipe.h"
#include "zstd-mt.h"

size_t zstdmt_errcode;

/* ------------------------------------------------------------------ errors (zstd-mt_common.c) */
unsigned ZSTDCB_isError(size_t code)
{
	return code > ZSTDCB_ERROR(maxCode);
}

const char *ZSTDCB_getErrorString(size_t code)
{
	/* strings of lib/zstd-mt_common.c:40-61 (init_missing and canceled have none there) */
	static const char *const codec[] = {
		"", "device: malformed record header", "device: bad zstd frame header",
		"device: malformed zstd block", "device: content size mismatch",
		"device: content checksum mismatch", "device: trailing bytes after frame",
		"device: unsupported zstd frame feature",
	};
	const size_t idx = (size_t)0 - code;
	if (zstdmt_errcode >= 1 && zstdmt_errcode <= 7 && idx == ZSTDCB_error_compression_library)
		return codec[zstdmt_errcode];
	/* init_missing sits at 2 in ZSTDCB_ErrorCode: the codes after it are one up against the shared table */
	if (idx < ZSTDCB_error_init_missing)
		return mt_error_name(idx);
	if (idx > ZSTDCB_error_init_missing && idx < ZSTDCB_error_canceled)
		return mt_error_name(idx - 1);
	return "Unspecified zstmt error code"; /* sic, zstd-mt_common.c:34 */
}

static int is_zstd_magic(const uint8_t *p) /* IsZstd_Magic, zstd-mt_decompress.c:146-153 */
{
	const uint32_t m = rd32(p);
	return m == ZSTDCB_MAGICNUMBER_V01 || (m >= ZSTDCB_MAGICNUMBER_MIN && m <= ZSTDCB_MAGICNUMBER_MAX);
}

/* Frame_Content_Size of a zstd frame header (RFC 8878 3.1.1.1), ~0 when absent / malformed */
static uint64_t zstd_content_size(const uint8_t *f, size_t n)
{
	if (n < 6 || rd32(f) != ZSTDCB_MAGICNUMBER_MAX)
		return ~(uint64_t)0;
	{
		const unsigned fhd = f[4], fcs = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
		const unsigned did_len = did == 3 ? 4 : did, fcs_len = fcs == 0 ? single : 1u << fcs;
		const size_t hp = 5 + (1 - single) + did_len;
		uint64_t c = 0;
		if (fcs_len == 0 || n < hp + fcs_len)
			return ~(uint64_t)0;
		for (unsigned k = 0; k < fcs_len; k++)
			c |= (uint64_t)f[hp + k] << (8 * k);
		return fcs == 1 ? c + 256 : c;
	}
}

/* ------------------------------------------------------------------ compression: mt_compress.inc */
/* default chunk = 1 << (windowLog[level] + 1), indexed by the level itself as in
 * zstd-mt_compress.c:116-127 (level 22 reads past that table there; 1 GiB here) */
static const int window_log[] = {19, 19, 20, 20, 20, 21, 21, 21, 21, 21, 22, 22,
				 22, 22, 22, 23, 23, 23, 23, 25, 26, 27, 29};

#define MTP(x) ZSTDCB_##x
#define MT_CODEC "zstd"
#define MT_LEVEL_OK(level) ((level) >= ZSTDCB_LEVEL_MIN && (level) <= ZSTDCB_LEVEL_MAX)
#define MT_DEFAULT_CHUNK(level) (1 << (window_log[level] + 1))
#define MT_SLOT_STRIDE(chunk) gpumt_zstd_slot_stride(chunk)
/* three device tiers for the level: gpumt_zstd_level_tier.  GPUMT_ZSTD_WIN=1 (exactly that) hands levels 10-22 to the
 * whole-chunk-window encoder instead, gpumt_zstd_compress_batch_win: same slots, same records, smaller frames; unset or
 * anything else, and below level 10, the call is the one above, byte for byte.  The variable is read per batch (the
 * launching thread alone reads it).  A weak reference, as in mt_lz4_plain.inc: a stand-in for the device boundary that
 * lacks the call leaves the engine on the table encoder */
extern __typeof__(gpumt_zstd_compress_batch_win) gpumt_zstd_compress_batch_win __attribute__((weak));
static int zstd_compress_batch(gpumt_ctx *g, const void *d_in, size_t n, size_t chunk, void *d_slots, size_t stride,
			       uint32_t *d_len, int level, int stream)
{
	const char *e = level >= 10 && gpumt_zstd_compress_batch_win ? getenv("GPUMT_ZSTD_WIN") : NULL;
	if (e && e[0] == '1' && !e[1])
		return gpumt_zstd_compress_batch_win(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
	return gpumt_zstd_compress_batch_level(g, d_in, n, chunk, d_slots, stride, d_len, level, stream);
}
#define MT_COMPRESS_BATCH zstd_compress_batch
#define MT_BATCH_UNIT(chunk) (chunk)
#define MT_C_DEVICE_ERROR compression_library
#define MT_C_NULL_CTX init_missing
#define MT_C_NULL_GET ZSTDCB_ERROR(init_missing) /* zstd-mt_compress.c:395-423 */
/* counters restart with every call (zstd-mt_compress.c:337-341) */
#define MT_COMPRESS_ENTER(ctx) \
	((ctx)->insize = (ctx)->outsize = (ctx)->frames = (ctx)->curframe = 0, zstdmt_errcode = 0, (size_t)0)

#include "mt_compress.inc"

/* ------------------------------------------------------------------ decompression: mt_records12.inc */
/* ZSTD_DStreamInSize() = 128 KiB + 3 per request, pieces of at most ZSTD_DStreamOutSize() = 128 KiB like the reference's */
#define ZSTD_IN_CHUNK 131075u
#define ZSTD_OUT_CHUNK 131072u

#define MT_ERRCODE zstdmt_errcode
#define MT_D_DEFAULT_INPUTSIZE (1024 * 512) /* zstd-mt_decompress.c:125-128 */
#define MT_D12_CHECK_SIZE_FIELD 0
#define MT_D12_STATUS_PRESET 1
/* GPUMT_ZSTD_REC_PAR=1 (exactly that) hands the batch to gpumt_zstd_decompress_batch_par, which decodes the records of
 * several blocks block-parallel: same records, statuses, sizes and bytes; unset or anything else, the call is the one below,
 * byte for byte.  Read per batch by the launching thread; a weak reference, as for the encoder above */
extern __typeof__(gpumt_zstd_decompress_batch_par) gpumt_zstd_decompress_batch_par __attribute__((weak));
static int zstd_decompress_batch(gpumt_ctx *g, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				 const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				 const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, int stream)
{
	const char *e = gpumt_zstd_decompress_batch_par ? getenv("GPUMT_ZSTD_REC_PAR") : NULL;
	if (e && e[0] == '1' && !e[1])
		return gpumt_zstd_decompress_batch_par(g, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes,
						       d_out_off, d_out_len, d_status, NULL, stream);
	return gpumt_zstd_decompress_batch(g, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					   d_out_len, d_status, stream);
}
#define MT_DECOMPRESS_BATCH zstd_decompress_batch
#define MT_FRAME_MAGIC ZSTDCB_MAGICNUMBER_MAX
#define MT_PLAIN_REQUEST(ctx) ((void)(ctx), (size_t)ZSTD_IN_CHUNK)
#define MT_PLAIN_PIECE(ctx) ((void)(ctx), (size_t)ZSTD_OUT_CHUNK)
#define MT_PLAIN_ENTER(ctx, nfirst) ((ctx)->insize += (nfirst))
#define MT_PLAIN_COUNT_FAILED_WRITE 0

#include "mt_frame_extent.h"

static size_t d12_out_size(const uint8_t *frame, uint32_t csize, uint64_t *osz, int *unsized)
{
	*osz = zstd_content_size(frame, csize);
	if (*osz == ~(uint64_t)0) {
		/* No content size: never written by zstd-mt, but pzstd-style writers that stream
		 * their frames do it, and the reference just grows its buffer (:499-522).  The block
		 * headers bound the content; the decoder replaces the capacity by the size. */
		uint64_t bound = 0;
		int sized = 0;
		const size_t fl = zstd_frame_extent(frame, csize, &bound, &sized);
		if (!fl || fl == EXTENT_INVALID || sized) {
			zstdmt_errcode = GPUMT_ST_BAD_FRAME;
			return ZSTDCB_ERROR(compression_library);
		}
		*osz = bound;
		*unsized = 1;
	}
	if (*osz > 0x7FFFFFFFull) {
		zstdmt_errcode = GPUMT_ST_UNSUPPORTED;
		return ZSTDCB_ERROR(compression_library);
	}
	return 0;
}

/* pt_decompress: any ZSTD error -> compression_library, code in the global (:534-536) */
static size_t d12_status_error(uint32_t st)
{
	zstdmt_errcode = st;
	return ZSTDCB_ERROR(compression_library);
}

static size_t plain_bad_frame(void)
{
	zstdmt_errcode = GPUMT_ST_BAD_FRAME;
	return ZSTDCB_ERROR(compression_library);
}

#include "mt_records12.inc"
#include "mt_zstd_plain.inc"

size_t ZSTDCB_decompressDCtx(ZSTDCB_DCtx *ctx, ZSTDCB_RdWr_t *rdwr)
{
	uint8_t sniff[16];
	ZSTDCB_Buffer b;
	int rv;

	if (!ctx)
		return ZSTDCB_ERROR(compressionParameter_unsupported); /* zstd-mt_decompress.c:703-704 */
	/* 16-byte sniff (:711-760) */
	b.buf = sniff;
	b.size = 16;
	b.allocated = 16;
	rv = rdwr->fn_read(rdwr->arg_read, &b);
	if (rv != 0)
		return mt_error(rv);
	if (b.size < 16) {
		if (b.size < 4 || !is_zstd_magic(sniff))
			return ZSTDCB_ERROR(data_error);
		if (b.size == 9)
			return 0; /* the 9-byte empty zstd frame: "create empty file" (:731-736) */
		return plain_decompress(ctx, rdwr, sniff, b.size, 1); /* a plain .zst shorter than the sniff */
	}
	ctx->insize += 16;
	ctx->have_hdr = 1;
	if (rd32(sniff) == ZSTDCB_MAGIC_SKIPPABLE && is_zstd_magic(sniff + 12)) {
		/* "pzstd style", what the compressor writes: the sniff is the first record's header + 4
		 * payload bytes (:251-284) */
		ctx->hdr_csize = rd32(sniff + 8);
		memcpy(ctx->first4, sniff + 12, 4);
		ctx->have_first4 = 1;
	} else if (is_zstd_magic(sniff) && rd32(sniff + 9) == ZSTDCB_MAGIC_SKIPPABLE) {
		/* old "zstdmt style": a 9-byte empty zstd frame, then ordinary records (:225-249).  The
		 * first header straddles the sniff: 5 more bytes complete it.  (insize: the reference
		 * counts the sniff twice here, :221 and :239; kept.) */
		uint8_t tail[5];
		b.buf = tail;
		b.size = 5;
		b.allocated = 5;
		rv = rdwr->fn_read(rdwr->arg_read, &b);
		if (rv != 0)
			return mt_error(rv);
		if (b.size != 5)
			return ZSTDCB_ERROR(data_error);
		ctx->insize += 16 + 5;
		ctx->hdr_csize = rd32(tail + 1);
		ctx->have_first4 = 0;
	} else {
		if (is_zstd_magic(sniff)) {
			ctx->insize -= 16; /* counted with the rest of the input below */
			return plain_decompress(ctx, rdwr, sniff, 16, 0); /* "some std zstd stream" (:755-759) */
		}
		return ZSTDCB_ERROR(data_error);
	}
	return d12_run(ctx, rdwr);
}
