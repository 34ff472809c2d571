/*
 * mt_compress.inc -- the compress half of every host engine: <PREFIX>_createCCtx / freeCCtx / Get*CCtx /
 * compressCCtx over gpumt_*.  The reference keeps one copy of this logic per codec (lib/lz4-mt_compress.c,
 * lib/zstd-mt_compress.c, lib/brotli-mt_compress.c, lib/snappy-mt_compress.c); here it is one text, included by
 * lz4mt_engine.c, zstdmt_engine.c and mt16_engine.inc (brotlimt_engine.c, snappymt_engine.c) with
 *
 *   MTP(x)                    <PREFIX>_##x  (MTP(ERROR)(name), MTP(Buffer), MTP(RdWr_t), MTP(THREAD_MAX), ...)
 *   MT_CODEC                  "lz4" / "zstd" / "brotli" / "snappy": names the trace lines (and mt16's default error string)
 *   MT_LEVEL_OK(level)        createCCtx's level check
 *   MT_DEFAULT_CHUNK(level)   chunk size for inputsize == 0
 *   MT_SLOT_STRIDE(chunk)     bytes a record can occupy
 *   MT_COMPRESS_BATCH         gpumt_*_compress_batch(g, in, n, chunk, slots, stride, lens, LEVEL, stream): a codec without
 *                             levels ignores LEVEL in its macro
 *   MT_BATCH_UNIT(chunk)      a device batch grows to zmt_batch_bytes_for(this) bytes
 *   MT_C_DEVICE_ERROR         error name for a device call that failed (compression_library / frame_compress)
 *   MT_C_NULL_CTX             error name compressCCtx(NULL, ...) returns
 *   MT_C_NULL_GET             what Get{Frames,Insize,Outsize}CCtx(NULL) return
 *   MT_COMPRESS_ENTER(ctx)    evaluated when compressCCtx starts: 0, or the error code to return at once
 *
 * pt_compress of the reference (lib/lz4-mt_compress.c:207-310, lib/zstd-mt_compress.c:208-392,
 * lib/brotli-mt_compress.c:194-318): one fn_read of exactly `inputsize` per chunk, EOF = a zero-length read once a
 * frame exists (an empty input still yields one record), a short read becomes a short record and the loop goes on;
 * one fn_write per record in order.  The records come from the device encoder (MT_COMPRESS_BATCH); `level` is
 * validated and sets the default chunk size where the reference does so.
 * Plain C, no HIP header.
 */
#include "mt_host.h"
#include "mt_pipe.h"

/* callback return value -> library error (reference mt_error, lz4-mt_compress.c:161-173, zstd-mt_compress.c:160-173,
 * brotli-mt_decompress.c:142-155; note that write failures go through the same mapping and so surface as read_fail) */
static size_t mt_error(int rv)
{
	switch (rv) {
	case -1:
		return MTP(ERROR)(read_fail);
	case -2:
		return MTP(ERROR)(canceled);
	case -3:
		return MTP(ERROR)(memory_allocation);
	}
	return MTP(ERROR)(read_fail);
}

struct cslot {
	dbuf in;      /* chunk data, H2D                       */
	dbuf slots;   /* device only: per-chunk records        */
	dbuf stream;  /* packed records, D2H                   */
	dbuf meta;    /* rec_len[n] u32 | pad | rec_off[n+1] u64, D2H */
	size_t n;     /* bytes in the batch                    */
	size_t nrec;
};

struct MTP(CCtx_s) {
	int level, threads, inputsize;
	size_t insize, outsize, curframe, frames; /* insize / frames: reader; outsize / curframe: writer */
	mt_gpus gpus; /* the devices the batch slots are dealt out to (mt_host.h) */
	struct cslot s[MT_NSLOT];
	MTP(RdWr_t) *io; /* callbacks of the running call */
	size_t maxrec;   /* records per device batch, grows (reader) */
};

MTP(CCtx) *MTP(createCCtx)(int threads, int level, int inputsize)
{
	MTP(CCtx) *ctx;
	if (threads < 1 || threads > MTP(THREAD_MAX))
		return NULL;
	if (!MT_LEVEL_OK(level))
		return NULL;
	if (inputsize < 0)
		return NULL;
	ctx = (MTP(CCtx) *)calloc(1, sizeof *ctx);
	if (!ctx)
		return NULL;
	ctx->level = level;
	ctx->threads = threads;
	ctx->inputsize = inputsize ? inputsize : MT_DEFAULT_CHUNK(level);
	if (mt_gpus_open(&ctx->gpus)) {
		free(ctx); /* no device: fail loudly, there is no CPU path */
		return NULL;
	}
	return ctx;
}

void MTP(freeCCtx)(MTP(CCtx) *ctx)
{
	if (!ctx)
		return;
	for (int i = 0; i < MT_NSLOT; i++)
		dbuf_free4(mt_gpu_of(&ctx->gpus, i), &ctx->s[i].in, &ctx->s[i].slots, &ctx->s[i].stream, &ctx->s[i].meta);
	mt_gpus_close(&ctx->gpus);
	free(ctx);
}

size_t MTP(GetFramesCCtx)(MTP(CCtx) *ctx) { return ctx ? ctx->curframe : MT_C_NULL_GET; }
size_t MTP(GetInsizeCCtx)(MTP(CCtx) *ctx) { return ctx ? ctx->insize : MT_C_NULL_GET; }
size_t MTP(GetOutsizeCCtx)(MTP(CCtx) *ctx) { return ctx ? ctx->outsize : MT_C_NULL_GET; }

/* offsets of the packed records: the second array of a slot's meta buffer (dev = 0: pinned mirror, 1: device) */
static uint64_t *c_rec_off(const struct cslot *s, int dev)
{
	return (uint64_t *)((uint8_t *)(dev ? s->meta.d : s->meta.h) + ((s->nrec * 4 + 15) & ~(size_t)15));
}

/*
 * Fill slot s with up to `maxrec` chunks.  Returns 0, or an error code; *eof is set when the
 * input is exhausted.  A short (non-zero) read is a short chunk and closes the batch, exactly
 * one fn_read per chunk as in pt_compress (lz4-mt_compress.c:256-277, zstd-mt_compress.c:250-277).
 */
static size_t c_read_batch(MTP(CCtx) *ctx, MTP(RdWr_t) *io, struct cslot *s, size_t maxrec, int *eof)
{
	const size_t chunk = (size_t)ctx->inputsize;
	s->n = 0;
	s->nrec = 0;
	while (s->nrec < maxrec) {
		MTP(Buffer) b;
		int rv;
		b.buf = (uint8_t *)s->in.h + s->n;
		b.size = chunk;
		b.allocated = chunk;
		rv = io->fn_read(io->arg_read, &b);
		if (rv != 0)
			return mt_error(rv);
		if (b.size == 0 && ctx->frames > 0) {
			*eof = 1;
			break;
		}
		if (b.size > chunk)
			return MTP(ERROR)(read_fail);
		ctx->insize += b.size;
		ctx->frames++;
		s->n += b.size;
		s->nrec++;
		if (b.size < chunk)
			break; /* ragged chunk (or the empty first read, which still yields one empty
				* frame): it must be the last one of this device batch; reading goes on
				* with the next batch, as the reference's loop does */
	}
	return 0;
}

static size_t c_launch(MTP(CCtx) *ctx, struct cslot *s)
{
	gpumt_ctx *g = mt_gpu_of(&ctx->gpus, (int)(s - ctx->s));
	const int ks = mt_stream_of(&ctx->gpus, (int)(s - ctx->s)); /* the slot's own kernel stream: batches overlap on the device */
	const size_t chunk = (size_t)ctx->inputsize;
	const size_t stride = MT_SLOT_STRIDE(chunk);
	uint32_t *d_len = (uint32_t *)s->meta.d;
	uint64_t *d_off = c_rec_off(s, 1);
	int rc = 0;
	if (s->n)
		rc |= gpumt_memcpy_h2d(g, s->in.d, s->in.h, s->n, 1);
	rc |= gpumt_stream_wait(g, ks, 1);
	/* the level the caller asked for reaches the encoder as the reference hands it to the codec library
	 * (lib/zstd-mt_compress.c:285, lib/brotli-mt_compress.c:269-272) */
	rc |= MT_COMPRESS_BATCH(g, s->in.d, s->n, chunk, s->slots.d, stride, d_len, ctx->level, ks);
	rc |= gpumt_lz4_compact(g, s->slots.d, stride, d_len, s->nrec, s->stream.d, d_off, ks);
	/* sizes, offsets and the packed records go to the pinned mirrors from the slot's own stream, the
	 * byte count of the records read on the device (d_off[nrec]): no host round trip in between, and
	 * the batches of the pipeline overlap (gpumt_push_host) */
	rc |= gpumt_push_host(g, s->meta.h, s->meta.d, ((s->nrec * 4 + 15) & ~(size_t)15) + (s->nrec + 1) * 8, NULL, ks);
	rc |= gpumt_push_host(g, s->stream.h, s->stream.d, s->stream.cap & ~(size_t)15, d_off + s->nrec, ks);
	return rc ? MTP(ERROR)(MT_C_DEVICE_ERROR) : 0;
}

/* ---- the three roles (mt_pipe.h) ---- */
static void cp_role_start(void *a) { mt_bind_near(&((MTP(CCtx) *)a)->gpus); }
static size_t cp_fill(void *a, int si, int *has_data, int *eof)
{
	MTP(CCtx) *ctx = (MTP(CCtx) *)a;
	struct cslot *s = &ctx->s[si];
	gpumt_ctx *g = mt_gpu_of(&ctx->gpus, si);
	const size_t chunk = (size_t)ctx->inputsize, stride = MT_SLOT_STRIDE(chunk);
	size_t lim = zmt_batch_bytes_for(MT_BATCH_UNIT(chunk)) / chunk, err;
	if (lim < 1)
		lim = 1;
	if (lim > BATCH_MAXREC)
		lim = BATCH_MAXREC;
	if (ctx->maxrec > lim)
		ctx->maxrec = lim;
	/* (re)size this slot for the current batch size; it is free: nothing of it is in flight */
	if (dbuf_want(g, &s->in, ctx->maxrec * chunk + 512, 1, 1) ||
	    dbuf_want(g, &s->slots, ctx->maxrec * stride, 0, 1) ||
	    dbuf_want(g, &s->stream, ctx->maxrec * stride + 512, 1, 1) ||
	    dbuf_want(g, &s->meta, ctx->maxrec * 12 + 64, 1, 1))
		return MTP(ERROR)(memory_allocation);
	err = c_read_batch(ctx, ctx->io, s, ctx->maxrec, eof);
	*has_data = s->nrec > 0;
	ctx->maxrec *= 4;
	return err;
}

static size_t cp_launch(void *a, int si)
{
	MTP(CCtx) *ctx = (MTP(CCtx) *)a;
	mt_trace_launch(&ctx->gpus, MT_CODEC "mt compress", si, ctx->s[si].nrec);
	size_t err = c_launch(ctx, &ctx->s[si]);
	if (!err && mt_slot_mark(&ctx->gpus, si, mt_stream_of(&ctx->gpus, si)))
		err = MTP(ERROR)(MT_C_DEVICE_ERROR);
	return err;
}

static size_t cp_complete(void *a, int si)
{
	MTP(CCtx) *ctx = (MTP(CCtx) *)a;
	struct cslot *s = &ctx->s[si];
	if (mt_slot_wait(&ctx->gpus, si)) /* record sizes and offsets are in host memory */
		return MTP(ERROR)(MT_C_DEVICE_ERROR);
	if ((size_t)c_rec_off(s, 0)[s->nrec] > s->stream.cap)
		return MTP(ERROR)(frame_compress);
	return 0;
}

static size_t cp_drain(void *a, int si)
{
	MTP(CCtx) *ctx = (MTP(CCtx) *)a;
	struct cslot *s = &ctx->s[si];
	const uint32_t *len = (const uint32_t *)s->meta.h;
	const uint64_t *off = c_rec_off(s, 0);
	for (size_t i = 0; i < s->nrec; i++) { /* pt_write: strictly in frame order */
		MTP(Buffer) b;
		int rv;
		b.buf = (uint8_t *)s->stream.h + off[i];
		b.size = len[i];
		b.allocated = len[i];
		rv = ctx->io->fn_write(ctx->io->arg_write, &b);
		if (rv != 0)
			return mt_error(rv);
		ctx->outsize += len[i];
		ctx->curframe++;
	}
	return 0;
}

size_t MTP(compressCCtx)(MTP(CCtx) *ctx, MTP(RdWr_t) *rdwr)
{
	static const mt_pipe_ops ops = {cp_fill, cp_launch, cp_complete, cp_drain, cp_role_start};
	size_t err;

	if (!ctx)
		return MTP(ERROR)(MT_C_NULL_CTX); /* lz4-mt_compress.c:317-318, zstd-mt_compress.c:327-328, brotli-mt_compress.c:325-326 */
	err = MT_COMPRESS_ENTER(ctx);
	if (err)
		return err;
	ctx->io = rdwr;
	ctx->maxrec = BATCH_MIN / (size_t)ctx->inputsize;
	if (ctx->maxrec < 1)
		ctx->maxrec = 1;
	err = mt_pipe_run_n(&ops, ctx, mt_nslot_for(ctx->gpus.n));
	mt_gpus_sync(&ctx->gpus);
	return err;
}
