/*
 * mt_records12.inc -- the decompress half of the codecs whose records carry a 12-byte header (lz4-mt, zstd-mt):
 * <PREFIX>_createDCtx / freeDCtx / Get*DCtx, the record pipeline (d12_run) and the writer of the plain-stream paths
 * (plain_write).  The reference has this logic once per codec (lib/lz4-mt_decompress.c:165-567,
 * lib/zstd-mt_decompress.c:209-549); here it is one text, included after mt_compress.inc by lz4mt_engine.c
 * and zstdmt_engine.c, which keep <PREFIX>_decompressDCtx (the sniff) to themselves and bring their plain path, block
 * by block, behind this file (mt_lz4_plain.inc, mt_zstd_plain.inc).  On top of mt_compress.inc's parameters:
 *
 *   MT_ERRCODE                  the library's global for a codec-level error (lz4mt_errcode / zstdmt_errcode)
 *   MT_D_DEFAULT_INPUTSIZE      createDCtx's inputsize for 0
 *   MT_D12_CHECK_SIZE_FIELD     1: a record header whose size field is not 4 is a data_error
 *   MT_D12_STATUS_PRESET        1: the status words are zeroed and uploaded before the kernel (a decoder that only
 *                               visits some of them)
 *   MT_DECOMPRESS_BATCH         gpumt_*_decompress_batch
 *   MT_FRAME_MAGIC              first four bytes of a frame the plain path takes
 *   MT_PLAIN_REQUEST(ctx)       bytes per fn_read of the plain path
 *   MT_PLAIN_PIECE(ctx)         largest fn_write of the plain path
 *   MT_PLAIN_ENTER(ctx, nfirst) the counters when the plain path starts
 *   MT_PLAIN_COUNT_FAILED_WRITE 1: outsize counts a piece whose fn_write failed
 *
 * and three hooks, defined by the including file before the include:
 *
 *   size_t d12_out_size(const uint8_t *frame, uint32_t csize, uint64_t *osz, int *unsized)
 *                               what a record decodes to; 0 or the error to return.  *unsized = 1: *osz is a capacity
 *                               and the decoder reports the size
 *   size_t d12_status_error(uint32_t st)        a record's device status (not GPUMT_ST_OK) -> library error
 *   size_t plain_bad_frame(void)                the error for bytes that cannot be split into frames
 *
 * Plain C, no HIP header.
 */
#include "mt_frame_extent.h"

struct dslot {
	dbuf in;     /* record bytes (headers included), H2D                                  */
	dbuf meta;   /* rec_off u64[n] | out_off u64[n+1] | rec_len u32[n] | out_len u32[n], H2D */
	dbuf status; /* u32[n], D2H                                                           */
	dbuf out;    /* decoded chunks, D2H                                                   */
	size_t nrec, in_bytes, out_bytes;
	int unsized; /* a frame of the batch states no content size: out_len holds capacities, read back */
};

struct MTP(DCtx_s) {
	int threads, inputsize;
	size_t budget; /* output bytes per device batch, grows from BATCH_MIN to zmt_batch_bytes_for(the largest record seen) */
	size_t big_out;
	size_t insize, outsize, curframe, frames;
	mt_gpus gpus; /* the devices the batch slots are dealt out to (mt_host.h) */
	struct dslot s[MT_NSLOT];
	MTP(RdWr_t) *io;
	/* a record header read ahead of its batch (or, zstd-mt, taken from the sniff) */
	int have_hdr;
	uint32_t hdr_csize;
	/* the next header is the stream's first and its magic went with the sniff (lz4-mt).  (The reference tests
	 * frames == 0 for this, lz4-mt_decompress.c:200, so its DCtx decodes one stream only -- the
	 * counters carry over and a second call fails with data_error; here a DCtx can be used again.) */
	int first_hdr;
	uint8_t first4[4]; /* first record: the 4 frame bytes that came with the sniff (zstd-mt) */
	int have_first4;
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
	ctx->inputsize = inputsize ? inputsize : MT_D_DEFAULT_INPUTSIZE;
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
		dbuf_free4(mt_gpu_of(&ctx->gpus, i), &ctx->s[i].in, &ctx->s[i].meta, &ctx->s[i].status, &ctx->s[i].out);
	mt_gpus_close(&ctx->gpus);
	free(ctx);
}

size_t MTP(GetFramesDCtx)(MTP(DCtx) *ctx) { return ctx ? ctx->curframe : 0; }
size_t MTP(GetInsizeDCtx)(MTP(DCtx) *ctx) { return ctx ? ctx->insize : 0; }
size_t MTP(GetOutsizeDCtx)(MTP(DCtx) *ctx) { return ctx ? ctx->outsize : 0; }

/* read one record header (pt_read, lz4-mt_decompress.c:192-236, zstd-mt_decompress.c:299-327): 0 = ok, *csize set;
 * eof flagged */
static size_t d_read_header(MTP(DCtx) *ctx, MTP(RdWr_t) *io, uint32_t *csize, int *eof)
{
	uint8_t hb[12];
	MTP(Buffer) b;
	int rv;
	const size_t skip = ctx->first_hdr ? 4 : 0; /* magic already consumed by the sniff */
	ctx->first_hdr = 0;
	b.buf = hb + skip;
	b.size = 12 - skip;
	b.allocated = 12 - skip;
	rv = io->fn_read(io->arg_read, &b);
	if (rv != 0)
		return mt_error(rv);
	if (!skip && b.size == 0) {
		*eof = 1;
		return 0;
	}
	if (b.size != 12 - skip)
		return MTP(ERROR)(read_fail);
	if (!skip && rd32(hb) != MT_MAGIC_SKIPPABLE)
		return MTP(ERROR)(data_error);
	if (MT_D12_CHECK_SIZE_FIELD && rd32(hb + 4) != 4)
		return MTP(ERROR)(data_error);
	ctx->insize += 12;
	*csize = rd32(hb + 8);
	return 0;
}

static size_t d_read_batch(MTP(DCtx) *ctx, MTP(RdWr_t) *io, struct dslot *s, int *eof)
{
	s->nrec = 0;
	s->unsized = 0;
	s->in_bytes = 0;
	s->out_bytes = 0;
	while (s->nrec < BATCH_MAXREC) {
		uint32_t csize = 0;
		uint64_t osz = 0;
		uint8_t *rec;
		MTP(Buffer) b;
		size_t err, skip = 0;
		int rv;
		if (ctx->have_hdr) {
			csize = ctx->hdr_csize;
		} else {
			err = d_read_header(ctx, io, &csize, eof);
			if (err)
				return err;
			if (*eof)
				break;
		}
		/* close the batch when it is full; the header just read waits for the next one */
		if (s->nrec && (s->in_bytes + 12 + (size_t)csize > s->in.cap - 512 || s->out_bytes >= ctx->budget)) {
			ctx->have_hdr = 1;
			ctx->hdr_csize = csize;
			break;
		}
		ctx->have_hdr = 0;
		/* a single record larger than the slot: grow (nothing is in flight in this slot) */
		if (s->in_bytes + 12 + (size_t)csize + 512 > s->in.cap &&
		    dbuf_grow_keep(mt_gpu_of(&ctx->gpus, (int)(s - ctx->s)), &s->in, s->in_bytes, s->in_bytes + 12 + (size_t)csize + 512))
			return MTP(ERROR)(memory_allocation);
		rec = (uint8_t *)s->in.h + s->in_bytes;
		mt_rec12_header(rec, csize); /* rebuild the 12-byte header in front of the payload: the device checks it too */
		if (ctx->have_first4) {
			/* first record: 4 payload bytes arrived with the 16-byte sniff (zstd-mt_decompress.c:262-270) */
			if (csize < 4)
				return MTP(ERROR)(data_error);
			memcpy(rec + 12, ctx->first4, 4);
			skip = 4;
			ctx->have_first4 = 0;
		}
		b.buf = rec + 12 + skip;
		b.size = csize - skip;
		b.allocated = b.size;
		rv = io->fn_read(io->arg_read, &b);
		if (rv != 0)
			return mt_error(rv);
		if (b.size != csize - skip)
			return MTP(ERROR)(data_error); /* "needed more bytes" */
		ctx->insize += b.size;
		ctx->frames++;
		err = d12_out_size(rec + 12, csize, &osz, &s->unsized);
		if (err)
			return err;
		if ((size_t)osz > ctx->big_out)
			ctx->big_out = (size_t)osz;
		m_rec_off(&s->meta, 0)[s->nrec] = s->in_bytes;
		m_rec_len(&s->meta, 0)[s->nrec] = 12 + csize;
		m_out_off(&s->meta, 0)[s->nrec] = s->out_bytes;
		m_out_len(&s->meta, 0)[s->nrec] = (uint32_t)osz;
		s->in_bytes += 12 + (size_t)csize;
		s->out_bytes += (size_t)osz;
		s->nrec++;
	}
	m_out_off(&s->meta, 0)[s->nrec] = s->out_bytes;
	return 0;
}

/* H2D, the decode kernel on stream ks and D2H on stream `back` for the batch the slot holds; out_len comes back too when
 * `sizes` is set (capacities -> decoded sizes) */
static int d_batch(gpumt_ctx *g, struct dslot *s, int up, int ks, int back, int sizes)
{
	int rc = 0;
	if (MT_D12_STATUS_PRESET)
		memset(s->status.h, 0, s->nrec * 4); /* GPUMT_ST_OK: the decode kernel only visits those */
	rc |= gpumt_memcpy_h2d(g, s->in.d, s->in.h, s->in_bytes, up);
	rc |= gpumt_memcpy_h2d(g, s->meta.d, s->meta.h, D_META_BYTES(BATCH_MAXREC), up);
	if (MT_D12_STATUS_PRESET)
		rc |= gpumt_memcpy_h2d(g, s->status.d, s->status.h, s->nrec * 4, up);
	if (ks != up)
		rc |= gpumt_stream_wait(g, ks, up);
	rc |= MT_DECOMPRESS_BATCH(g, s->in.d, s->in_bytes, m_rec_off(&s->meta, 1), m_rec_len(&s->meta, 1), s->nrec,
				  s->out.d, s->out_bytes, m_out_off(&s->meta, 1), m_out_len(&s->meta, 1),
				  (uint32_t *)s->status.d, ks);
	if (back != ks)
		rc |= gpumt_stream_wait(g, back, ks);
	rc |= gpumt_memcpy_d2h(g, s->status.h, s->status.d, s->nrec * 4, back);
	if (sizes)
		rc |= gpumt_memcpy_d2h(g, m_out_len(&s->meta, 0), m_out_len(&s->meta, 1), s->nrec * 4, back);
	if (s->out_bytes)
		rc |= gpumt_memcpy_d2h(g, s->out.h, s->out.d, s->out_bytes, back);
	return rc;
}

static size_t d_launch(MTP(DCtx) *ctx, struct dslot *s)
{
	gpumt_ctx *g = mt_gpu_of(&ctx->gpus, (int)(s - ctx->s));
	if (dbuf_want(g, &s->out, s->out_bytes + 64, 1, 1) || dbuf_want(g, &s->status, s->nrec * 4 + 64, 1, 1))
		return MTP(ERROR)(memory_allocation);
	/* each batch slot launches on its own kernel stream (4 + slot): the decoders are bound by the
	 * latency of a record, so the batches of the pipeline must overlap on the device */
	return d_batch(g, s, 1, mt_stream_of(&ctx->gpus, (int)(s - ctx->s)), 2, s->unsized) ? MTP(ERROR)(compression_library) : 0;
}

static void dp_role_start(void *a) { mt_bind_near(&((MTP(DCtx) *)a)->gpus); }
static size_t dp_fill(void *a, int si, int *has_data, int *eof)
{
	MTP(DCtx) *ctx = (MTP(DCtx) *)a;
	struct dslot *s = &ctx->s[si];
	size_t err;
	/* input slot sized for the batch budget (compressed data is never larger than that plus
	 * per-record overhead); the slot is free here */
	if (dbuf_want(mt_gpu_of(&ctx->gpus, si), &s->in, ctx->budget + (ctx->budget >> 3) + 4096, 1, 1) ||
	    dbuf_want(mt_gpu_of(&ctx->gpus, si), &s->meta, D_META_BYTES(BATCH_MAXREC), 1, 1))
		return MTP(ERROR)(memory_allocation);
	err = d_read_batch(ctx, ctx->io, s, eof);
	*has_data = s->nrec > 0;
	if (ctx->budget < zmt_batch_bytes_for(ctx->big_out))
		ctx->budget *= 4;
	return err;
}

static size_t dp_launch(void *a, int si)
{
	MTP(DCtx) *ctx = (MTP(DCtx) *)a;
	mt_trace_launch(&ctx->gpus, MT_CODEC "mt decompress", si, ctx->s[si].nrec);
	size_t err = d_launch(ctx, &ctx->s[si]);
	if (!err && mt_slot_mark(&ctx->gpus, si, 2))
		err = MTP(ERROR)(compression_library);
	return err;
}

static size_t dp_complete(void *a, int si)
{
	return mt_slot_wait(&((MTP(DCtx) *)a)->gpus, si) ? MTP(ERROR)(compression_library) : 0;
}

static size_t dp_drain(void *a, int si)
{
	MTP(DCtx) *ctx = (MTP(DCtx) *)a;
	struct dslot *s = &ctx->s[si];
	const uint32_t *st = (const uint32_t *)s->status.h;
	for (size_t i = 0; i < s->nrec; i++) {
		MTP(Buffer) b;
		int rv;
		if (st[i] != GPUMT_ST_OK)
			return d12_status_error(st[i]);
		b.buf = (uint8_t *)s->out.h + m_out_off(&s->meta, 0)[i];
		b.size = m_out_len(&s->meta, 0)[i];
		b.allocated = b.size;
		rv = ctx->io->fn_write(ctx->io->arg_write, &b);
		if (rv != 0)
			return mt_error(rv);
		ctx->outsize += b.size;
		ctx->curframe++;
	}
	return 0;
}

/* the records that follow the sniff, through the pipeline; the caller has set have_hdr / first_hdr / first4 */
static size_t d12_run(MTP(DCtx) *ctx, MTP(RdWr_t) *rdwr)
{
	static const mt_pipe_ops ops = {dp_fill, dp_launch, dp_complete, dp_drain, dp_role_start};
	size_t err;
	ctx->io = rdwr;
	ctx->budget = BATCH_MIN;
	ctx->big_out = 0;
	/* threads == 1: every callback on the calling thread, as the reference (its single-thread path) */
	err = ctx->threads == 1 ? mt_pipe_run_inline(&ops, ctx) : mt_pipe_run_n(&ops, ctx, mt_nslot_for(ctx->gpus.n));
	mt_gpus_sync(&ctx->gpus);
	return err;
}

/* =================================================================== plain streams
 * A stream that starts with a frame of the codec instead of a skippable record is decoded by the reference on one
 * thread with the codec's streaming decoder (st_decompress, lz4-mt_decompress.c:391-483, zstd-mt_decompress.c:552-687):
 * files of the lz4 / zstd tools and libraries, any number of frames, possibly without a content size and with
 * skippable frames in between.  Here the input is read about one batch ahead (same request sizes as the reference),
 * walked block by block on the host and decoded by the device's block-level calls (mt_lz4_plain.inc,
 * mt_zstd_plain.inc).  Output leaves in pieces like the reference's; GetFrames stays 0 as in the reference
 * (st_decompress counts no frames). */
static size_t plain_write(MTP(DCtx) *ctx, MTP(RdWr_t) *io, const uint8_t *p, size_t n)
{
	const size_t piece = MT_PLAIN_PIECE(ctx);
	while (n) {
		MTP(Buffer) b;
		const size_t k = n < piece ? n : piece;
		int rv;
		b.buf = (void *)p;
		b.size = k;
		b.allocated = k;
		rv = io->fn_write(io->arg_write, &b);
		if (rv != 0 && !MT_PLAIN_COUNT_FAILED_WRITE)
			return mt_error(rv);
		ctx->outsize += k;
		if (rv != 0)
			return mt_error(rv);
		p += k;
		n -= k;
	}
	return 0;
}
