/*
 * mt16_engine.inc -- the host side of the codecs whose records carry a 16-byte header (brotli-mt,
 * snappy-mt): <PREFIX>_* over gpumt_*.  The reference keeps one copy of this logic per codec
 * (lib/brotli-mt_{compress,decompress}.c, lib/snappy-mt_{compress,decompress}.c: the same file with
 * the codec call and three constants changed); here it is one text, included by brotlimt_engine.c and
 * snappymt_engine.c with
 *
 *   MTP(x)                    <PREFIX>_##x
 *   MT_CODEC                  "brotli" / "snappy" (the default error string, the trace lines)
 *   MT_LEVEL_OK(level)        createCCtx's level check
 *   MT_DEFAULT_CHUNK(level)   chunk size for inputsize == 0
 *   MT_SLOT_STRIDE(chunk)     bytes a record can occupy
 *   MT_COMPRESS_BATCH         gpumt_*_compress_batch(g, in, n, chunk, slots, stride, lens, LEVEL, stream): a codec without
 *                             levels ignores LEVEL in its macro
 *   MT_DECOMPRESS_BATCH       gpumt_*_decompress_batch
 *   MT_CAP_FROM_PREAMBLE      0: a record's output capacity is hint << 16 (brotli-mt_decompress.c:236-239)
 *                             1: it is the varint in front of the stream (snappy-mt_decompress.c:262-267;
 *                                the hint is not read)
 *
 * Decompression follows the callback-visible behaviour of the reference
 * (lib/brotli-mt_decompress.c:187-454, lib/snappy-mt_decompress.c:185-460): a 4-byte sniff that must be
 * the skippable magic, 12 more header bytes for the first record and 16 for every later one, the
 * payload in one read, one fn_write per record in order; a stream that does not decode into its
 * capacity fails with frame_decompress.  Records move through the same three-role batch pipeline as
 * the other codecs (mt_pipe.h): H2D / decode kernel / D2H on three streams.
 * Compression: pt_compress behaviour over the device encoder, mt_compress.inc (shared with lz4mt_engine.c and
 * zstdmt_engine.c).
 * Plain C, no HIP header.
 */
#include "mt_host.h"
#include "mt_pipe.h"

/* ------------------------------------------------------------------ errors (brotli-mt_common.c) */
unsigned MTP(isError)(size_t code)
{
	return code > MTP(ERROR)(maxCode);
}

const char *MTP(getErrorString)(size_t code)
{
	/* strings of lib/brotli-mt_common.c:37-57: compression_library and canceled have none there */
	const size_t idx = (size_t)0 - code;
	return idx < MTP(error_compression_library) ? mt_error_name(idx) : "Unspecified " MT_CODEC " error code";
}

/* =================================================================== compression
 * mt_compress.inc, with what brotli-mt and snappy-mt have in common.  One fn_write per record: 16-byte header
 * (hint = 64 KiB units of output, lib/brotli-mt_compress.c:294-304) + one codec stream; the streams are
 * decompress-identical to the input. */
#define MT_BATCH_UNIT(chunk) (chunk)
#define MT_C_DEVICE_ERROR frame_compress
#define MT_C_NULL_CTX compressionParameter_unsupported /* brotli-mt_compress.c:325-326 */
#define MT_C_NULL_GET 0
#define MT_COMPRESS_ENTER(ctx) ((void)(ctx), (size_t)0) /* counters carry over from the last call */

#include "mt_compress.inc"

/* =================================================================== decompression */
struct dslot {
	dbuf in;   /* record payloads back to back, H2D                                              */
	dbuf meta; /* rec_off u64[n] | out_off u64[n+1] | rec_len u32[n] | out_cap u32[n], H2D       */
	dbuf res;  /* out_len u32[n] | status u32[n], D2H                                            */
	dbuf out;  /* one slot of hint << 16 bytes per record, D2H                                   */
	size_t nrec, in_bytes, out_bytes;
};

struct MTP(DCtx_s) {
	int threads, inputsize;
	size_t budget;
	size_t insize, outsize, curframe, frames;
	mt_gpus gpus; /* the devices the batch slots are dealt out to (mt_host.h) */
	struct dslot s[MT_NSLOT];
	MTP(RdWr_t) *io;
	int have_hdr; /* a record header read ahead of its batch */
	uint32_t hdr_csize, hdr_hint;
	int first; /* the next header is the first one: its magic came with the sniff */
};

MTP(DCtx) *MTP(createDCtx)(int threads, int inputsize)
{
	MTP(DCtx) *ctx;
	if (threads < 1 || threads > MTP(THREAD_MAX))
		return NULL;
	ctx = (MTP(DCtx) *)calloc(1, sizeof *ctx);
	if (!ctx)
		return NULL;
	ctx->threads = threads;
	ctx->inputsize = inputsize ? inputsize : 1024 * 64; /* brotli-mt_decompress.c:110-113, snappy-mt: :101-104 */
	if (mt_gpus_open(&ctx->gpus)) {
		free(ctx);
		return NULL;
	}
	return ctx;
}

void MTP(freeDCtx)(MTP(DCtx) *ctx)
{
	if (!ctx)
		return;
	for (int i = 0; i < MT_NSLOT; i++)
		dbuf_free4(mt_gpu_of(&ctx->gpus, i), &ctx->s[i].in, &ctx->s[i].meta, &ctx->s[i].res, &ctx->s[i].out);
	mt_gpus_close(&ctx->gpus);
	free(ctx);
}

size_t MTP(GetFramesDCtx)(MTP(DCtx) *ctx) { return ctx ? ctx->curframe : 0; }
size_t MTP(GetInsizeDCtx)(MTP(DCtx) *ctx) { return ctx ? ctx->insize : 0; }
size_t MTP(GetOutsizeDCtx)(MTP(DCtx) *ctx) { return ctx ? ctx->outsize : 0; }

/* the meta arrays of mt_host.h, the fourth one holding capacities here; the decoder's answers are in `res` */
static uint32_t *m_out_cap(const dbuf *meta, int dev) { return m_out_len(meta, dev); }
static uint32_t *r_out_len(struct dslot *s, int dev) { return (uint32_t *)(dev ? s->res.d : s->res.h); }
static uint32_t *r_status(struct dslot *s, int dev) { return r_out_len(s, dev) + BATCH_MAXREC; }

/* next record header (pt_read, brotli-mt_decompress.c:193-240): 12 bytes after the sniff, else 16 */
static size_t d_read_header(MTP(DCtx) *ctx, MTP(RdWr_t) *io, uint32_t *csize, uint32_t *hint, int *eof)
{
	uint8_t hb[16];
	MTP(Buffer) b;
	int rv;
	const size_t want = ctx->first ? 12 : 16;
	b.buf = ctx->first ? hb + 4 : hb;
	b.size = want;
	b.allocated = want;
	rv = io->fn_read(io->arg_read, &b);
	if (rv != 0)
		return mt_error(rv);
	if (!ctx->first && b.size == 0) {
		*eof = 1;
		return 0;
	}
	if (b.size != want)
		return MTP(ERROR)(read_fail);
	if (!ctx->first && rd32(hb) != MTP(MAGIC_SKIPPABLE))
		return MTP(ERROR)(data_error);
	ctx->first = 0;
	if (rd32(hb + 4) != 8)
		return MTP(ERROR)(data_error);
	if (((uint32_t)hb[12] | (uint32_t)hb[13] << 8) != MTP(MAGICNUMBER))
		return MTP(ERROR)(data_error);
	ctx->insize += 16;
	*csize = rd32(hb + 8);
	*hint = (uint32_t)hb[14] | (uint32_t)hb[15] << 8;
	return 0;
}

/*
 * One wave decodes one record, and a 1 MiB record keeps it busy for ~165 ms whatever else runs, so
 * the device is only full with thousands of records in flight: the output budget of a batch grows
 * to four times the common batch size (1 GiB by default = 1 024 records of the level-1 chunk size).
 * Compressed bytes a batch may hold: the budget plus an eighth (records that did not shrink).
 */
#define D_BATCH_BYTES (4 * BATCH_BYTES)
#define D_IN_LIMIT(budget) ((budget) + ((budget) >> 3))

static size_t d_read_batch(MTP(DCtx) *ctx, MTP(RdWr_t) *io, struct dslot *s, int *eof)
{
	s->nrec = 0;
	s->in_bytes = 0;
	s->out_bytes = 0;
	while (s->nrec < BATCH_MAXREC) {
		uint32_t csize = 0, hint = 0;
		MTP(Buffer) b;
		size_t err, cap;
		int rv;
		if (ctx->have_hdr) {
			csize = ctx->hdr_csize;
			hint = ctx->hdr_hint;
		} else {
			err = d_read_header(ctx, io, &csize, &hint, eof);
			if (err)
				return err;
			if (*eof)
				break;
		}
		/* what the record may decode to: the hint -- or, where the reference sizes the output from
		 * the stream itself, not known before the payload is here: the batch then closes on what
		 * it holds already and the capacity is read below */
		cap = MT_CAP_FROM_PREAMBLE ? 0 : (size_t)hint << 16;
		if (s->nrec && (s->in_bytes + (size_t)csize > D_IN_LIMIT(ctx->budget) || s->out_bytes + cap > ctx->budget ||
				(MT_CAP_FROM_PREAMBLE && s->out_bytes >= ctx->budget))) {
			ctx->have_hdr = 1;
			ctx->hdr_csize = csize;
			ctx->hdr_hint = hint;
			break;
		}
		ctx->have_hdr = 0;
		if (s->in_bytes + (size_t)csize + 512 > s->in.cap) {
			/* the record buffer starts at half the output budget (text shrinks more than 2:1) and
			 * doubles when a batch needs more */
			size_t want = s->in_bytes + (size_t)csize + 512;
			if (want < 2 * s->in.cap)
				want = 2 * s->in.cap;
			if (dbuf_grow_keep(mt_gpu_of(&ctx->gpus, (int)(s - ctx->s)), &s->in, s->in_bytes, want))
				return MTP(ERROR)(memory_allocation);
		}
		b.buf = (uint8_t *)s->in.h + s->in_bytes;
		b.size = csize;
		b.allocated = csize;
		rv = io->fn_read(io->arg_read, &b);
		if (rv != 0)
			return mt_error(rv);
		if (b.size != csize)
			return MTP(ERROR)(data_error); /* "needed more bytes!" (:259-260) */
		ctx->insize += csize;
		ctx->frames++;
#if MT_CAP_FROM_PREAMBLE
		{
			/* snappy_uncompressed_length (snappy-mt_decompress.c:262-267): a varint of at most 32 bits.
			 * The reference allocates whatever it says; a stream cannot decode to more than 64 bytes per
			 * 3 of its own (a copy element), so a larger claim is malformed without looking further --
			 * such a record gets capacity 0 and the decoder's verdict (frame_decompress) */
			const uint8_t *pp = (const uint8_t *)s->in.h + s->in_bytes;
			uint64_t v = 0;
			int ok = 0;
			for (uint32_t k = 0; k < 5 && k < csize; k++) {
				v |= (uint64_t)(pp[k] & 127u) << (7 * k);
				if (pp[k] < 128) {
					ok = 1;
					break;
				}
			}
			/* (and no chunk is larger than an int: createCCtx's inputsize) */
			cap = ok && v <= 0x7FFFFFFFull && v <= (uint64_t)csize * 22u + 64u ? (size_t)v : 0;
		}
#endif
		m_rec_off(&s->meta, 0)[s->nrec] = s->in_bytes;
		m_rec_len(&s->meta, 0)[s->nrec] = csize;
		m_out_off(&s->meta, 0)[s->nrec] = s->out_bytes;
		m_out_cap(&s->meta, 0)[s->nrec] = (uint32_t)cap;
		s->in_bytes += csize;
		s->out_bytes += cap;
		s->nrec++;
	}
	m_out_off(&s->meta, 0)[s->nrec] = s->out_bytes;
	return 0;
}

static size_t d_launch(MTP(DCtx) *ctx, struct dslot *s)
{
	gpumt_ctx *g = mt_gpu_of(&ctx->gpus, (int)(s - ctx->s));
	/* each batch slot launches on its own kernel stream (4 + slot): the decoders are bound by the
	 * latency of a record, so the batches of the pipeline must overlap on the device */
	const int ks = mt_stream_of(&ctx->gpus, (int)(s - ctx->s));
	int rc = 0;
	if (dbuf_want(g, &s->out, s->out_bytes + 64, 1, 1) || dbuf_want(g, &s->res, BATCH_MAXREC * 8 + 64, 1, 1))
		return MTP(ERROR)(memory_allocation);
	rc |= gpumt_memcpy_h2d(g, s->in.d, s->in.h, s->in_bytes + 256, 1);
	rc |= gpumt_memcpy_h2d(g, s->meta.d, s->meta.h, D_META_BYTES(BATCH_MAXREC), 1);
	rc |= gpumt_stream_wait(g, ks, 1);
	rc |= MT_DECOMPRESS_BATCH(g, s->in.d, m_rec_off(&s->meta, 1), m_rec_len(&s->meta, 1), s->nrec, s->out.d,
					    m_out_off(&s->meta, 1), m_out_cap(&s->meta, 1), r_out_len(s, 1), r_status(s, 1), ks);
	rc |= gpumt_stream_wait(g, 2, ks);
	rc |= gpumt_memcpy_d2h(g, s->res.h, s->res.d, BATCH_MAXREC * 8, 2);
	if (s->out_bytes)
		rc |= gpumt_memcpy_d2h(g, s->out.h, s->out.d, s->out_bytes, 2);
	return rc ? MTP(ERROR)(frame_decompress) : 0;
}

static void dp_role_start(void *a) { mt_bind_near(&((MTP(DCtx) *)a)->gpus); }
static size_t dp_fill(void *a, int si, int *has_data, int *eof)
{
	MTP(DCtx) *ctx = (MTP(DCtx) *)a;
	struct dslot *s = &ctx->s[si];
	size_t err;
	if (dbuf_want(mt_gpu_of(&ctx->gpus, (int)(s - ctx->s)), &s->in, (ctx->budget >> 1) + 4096, 1, 1) ||
	    dbuf_want(mt_gpu_of(&ctx->gpus, (int)(s - ctx->s)), &s->meta, D_META_BYTES(BATCH_MAXREC), 1, 1))
		return MTP(ERROR)(memory_allocation);
	err = d_read_batch(ctx, ctx->io, s, eof);
	*has_data = s->nrec > 0;
	if (ctx->budget < D_BATCH_BYTES)
		ctx->budget *= 4;
	return err;
}

static size_t dp_launch(void *a, int si)
{
	MTP(DCtx) *ctx = (MTP(DCtx) *)a;
	mt_trace_launch(&ctx->gpus, MT_CODEC "mt decompress", si, ctx->s[si].nrec);
	size_t err = d_launch(ctx, &ctx->s[si]);
	if (!err && mt_slot_mark(&ctx->gpus, si, 2))
		err = MTP(ERROR)(frame_decompress);
	return err;
}

static size_t dp_complete(void *a, int si)
{
	return mt_slot_wait(&((MTP(DCtx) *)a)->gpus, si) ? MTP(ERROR)(frame_decompress) : 0;
}

static size_t dp_drain(void *a, int si)
{
	MTP(DCtx) *ctx = (MTP(DCtx) *)a;
	struct dslot *s = &ctx->s[si];
	const uint32_t *st = r_status(s, 0), *ol = r_out_len(s, 0);
	for (size_t i = 0; i < s->nrec; i++) {
		MTP(Buffer) b;
		int rv;
		if (st[i] != GPUMT_ST_OK)
			return MTP(ERROR)(frame_decompress); /* pt_decompress :348-351 */
		b.buf = (uint8_t *)s->out.h + m_out_off(&s->meta, 0)[i];
		b.size = ol[i];
		b.allocated = m_out_cap(&s->meta, 0)[i];
		rv = ctx->io->fn_write(ctx->io->arg_write, &b);
		if (rv != 0)
			return mt_error(rv);
		ctx->outsize += b.size;
		ctx->curframe++;
	}
	return 0;
}

size_t MTP(decompressDCtx)(MTP(DCtx) *ctx, MTP(RdWr_t) *rdwr)
{
	uint8_t sniff[4];
	MTP(Buffer) b;
	static const mt_pipe_ops ops = {dp_fill, dp_launch, dp_complete, dp_drain, dp_role_start};
	size_t err;
	int rv;

	if (!ctx)
		return MTP(ERROR)(compressionParameter_unsupported); /* brotli-mt_decompress.c:387-388 */
	/* 4-byte sniff: only the skippable-frame layout exists for brotli (:397-407) */
	b.buf = sniff;
	b.size = 4;
	b.allocated = 4;
	rv = rdwr->fn_read(rdwr->arg_read, &b);
	if (rv != 0)
		return mt_error(rv);
	if (b.size != 4)
		return MTP(ERROR)(data_error);
	if (rd32(sniff) != MTP(MAGIC_SKIPPABLE))
		return MTP(ERROR)(data_error);
	ctx->first = 1;
	ctx->have_hdr = 0;
	ctx->budget = BATCH_MIN;
	ctx->io = rdwr;
	/* threads == 1: every callback on the calling thread, as the reference (its single-thread path) */
	err = ctx->threads == 1 ? mt_pipe_run_inline(&ops, ctx) : mt_pipe_run_n(&ops, ctx, mt_nslot_for(ctx->gpus.n));
	mt_gpus_sync(&ctx->gpus);
	return err;
}
