/*
 * mt_lz4_plain.inc -- the plain .lz4 path of LZ4MT_decompressDCtx: a stream that starts with an LZ4 frame instead of a
 * skippable record (files of the lz4 tool and of liblz4 callers).  The reference decodes it on one thread with streaming
 * LZ4F_decompress (st_decompress, lib/lz4-mt_decompress.c:391-483), at any size.  Here the frame is not the unit of
 * work, the block is: a state machine walks the bytes read so far (frame header, block header, block body + block
 * checksum, end mark, content checksum; skippable frames in between are dropped), every block that is complete in the
 * buffer goes into the batch's block table, and the device decodes the table with gpumt_lz4_decompress_blocks --
 * independent blocks one wave each, the blocks of a linked frame in order by one wave (or, under GPUMT_LZ4_RUN_PAR=1,
 * side by side with gpumt_lz4_decompress_blocks_par; under GPUMT_LZ4_BLOCK_SEG=1 every block in segments side by side
 * with gpumt_lz4_decompress_blocks_seg), with the last 64 KiB of the frame's earlier output copied in
 * front of the batch's output.  Neither mode needs the whole frame: host memory is
 * about two batches of input plus one block whatever the frame size, and there is no limit on a frame's size.
 * The content checksum is one serial XXH32 chain over the frame; its state lives on the device, is continued batch by
 * batch (gpumt_xxh32_carry) on stream PL_XS and is settled when the batch's buffers are taken again, so it runs under
 * the next batch's read, decode and write.  One batch at a time otherwise: read, decode, write on the calling thread.
 * As with the reference's streaming decoder, output of earlier batches (and of a batch whose checksum later turns out
 * wrong) may have been written when an error surfaces; the return value is what counts.
 * Included by lz4mt_engine.c behind mt_records12.inc (the context, plain_write).  Plain C, no HIP header.
 */
#include <time.h>

/* The device calls that only this path uses are weak references here.  In the library they bind to gpumt.hip like every
 * other call; a stand-in for the device boundary that does not provide them (the plain-C one the host engines are
 * linked with for ThreadSanitizer runs, which only ever feeds records) still links, and this path then fails with
 * compression_library -- an error, not another way to decode. */
extern __typeof__(gpumt_lz4_decompress_blocks) gpumt_lz4_decompress_blocks __attribute__((weak));
extern __typeof__(gpumt_lz4_decompress_blocks_par) gpumt_lz4_decompress_blocks_par __attribute__((weak));
extern __typeof__(gpumt_lz4_decompress_blocks_seg) gpumt_lz4_decompress_blocks_seg __attribute__((weak));
extern __typeof__(gpumt_lz4_pack_runs) gpumt_lz4_pack_runs __attribute__((weak));
extern __typeof__(gpumt_xxh32_carry) gpumt_xxh32_carry __attribute__((weak));
extern __typeof__(gpumt_memcpy_d2d) gpumt_memcpy_d2d __attribute__((weak));

#define PL_MAXB BATCH_MAXREC /* blocks, runs, frame segments of one batch */
#define PL_HIST 65536u
#define PL_XS 3 /* the stream of the carried content checksum */
#define PL_PAR_DEFAULT 0 /* linked runs block-parallel unless GPUMT_LZ4_RUN_PAR says otherwise */

/* the tables of a batch in the slot's `meta` buffer (pinned mirror and device copy alike) */
#define PL_OFF_BLOCKS 0
#define PL_OFF_RUNS (PL_OFF_BLOCKS + sizeof(gpumt_lz4_block) * PL_MAXB)
#define PL_OFF_JOBS (PL_OFF_RUNS + sizeof(gpumt_lz4_run) * PL_MAXB)
#define PL_OFF_BLKLEN (PL_OFF_JOBS + sizeof(gpumt_xxh32_job) * PL_MAXB)
#define PL_OFF_RUNLEN (PL_OFF_BLKLEN + 4 * PL_MAXB)
#define PL_OFF_STATUS (PL_OFF_RUNLEN + 4 * PL_MAXB)
#define PL_OFF_DIGEST (PL_OFF_STATUS + 4 * PL_MAXB)
#define PL_OFF_VERDICT (PL_OFF_DIGEST + 4 * PL_MAXB)
#define PL_OFF_PACKOFF (PL_OFF_VERDICT + 4 * PL_MAXB)
#define PL_OFF_BLKSEG (PL_OFF_PACKOFF + 8 * (PL_MAXB + 1))
#define PL_META_BYTES (PL_OFF_BLKSEG + 4 * PL_MAXB + 64)
#define PL_AT(type, meta, dev, off) ((type *)((uint8_t *)((dev) ? (meta)->d : (meta)->h) + (off)))

struct pl_frame { /* the frame the walker is inside of */
	int open, indep, bchk, cchk, has_csize;
	uint32_t blkmax;
	uint64_t csize, produced; /* produced: content bytes of the batches before this one */
};

struct pl_seg { /* the part of one frame a batch holds */
	uint32_t run0, nrun;
	int first, last, cchk, has_csize;
	uint32_t expect;
	uint64_t csize, before; /* before: the frame's content ahead of this batch */
};

/* XXH32 (seed 0) of up to 15 bytes: the frame descriptor's checksum byte is bits 8..15 of it */
static uint32_t pl_xxh32_short(const uint8_t *p, size_t len)
{
	uint32_t h = 374761393u + (uint32_t)len;
	while (len >= 4) {
		h += rd32(p) * 3266489917u;
		h = (h << 17 | h >> 15) * 668265263u;
		p += 4;
		len -= 4;
	}
	while (len--) {
		h += *p++ * 374761393u;
		h = (h << 11 | h >> 21) * 2654435761u;
	}
	h ^= h >> 15;
	h *= 2246822519u;
	h ^= h >> 13;
	h *= 3266489917u;
	h ^= h >> 16;
	return h;
}

static double pl_now(void)
{
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* the verdicts of the checksum jobs slot b left behind: waited for before the slot's buffers are taken again */
static size_t pl_settle(MTP(DCtx) *ctx, gpumt_ctx *g, int b, size_t *pend)
{
	size_t err = 0;
	if (!pend[b])
		return 0;
	if (gpumt_mark_sync(g, b))
		err = MTP(ERROR)(compression_library);
	for (size_t j = 0; j < pend[b] && !err; j++) {
		const uint32_t v = PL_AT(uint32_t, &ctx->s[b].meta, 0, PL_OFF_VERDICT)[j];
		if (v != GPUMT_ST_OK) {
			MT_ERRCODE = v;
			err = MTP(ERROR)(compression_library);
		}
	}
	pend[b] = 0;
	return err;
}

/* first[0..nfirst) came with the sniff */
static size_t lz4_plain_decompress(MTP(DCtx) *ctx, MTP(RdWr_t) *io, const uint8_t *first, size_t nfirst)
{
	const size_t req = MT_PLAIN_REQUEST(ctx);
	/* output a batch may decode to: as the input budget allows at 4:1, at most 1 GiB (positions inside a run are 32 bits) */
	const size_t out_budget = 4 * BATCH_BYTES < ((size_t)1 << 30) ? 4 * BATCH_BYTES : (size_t)1 << 30;
	size_t cap = req + nfirst, n = nfirst, ip = 0, err = 0, need = 4, pend[2] = {0, 0};
	uint8_t *raw = (uint8_t *)malloc(cap);
	int eof = 0, batch = 0, xs = 0, pack_busy = 0, done = 0;
	uint64_t skip_left = 0;
	struct pl_frame fr;
	struct pl_seg *segs = (struct pl_seg *)malloc(sizeof(struct pl_seg) * PL_MAXB);
	gpumt_ctx *g = mt_gpu_of(&ctx->gpus, 0);
	uint32_t *d_states = (uint32_t *)gpumt_malloc(g, 2 * GPUMT_XXH32_STATE_WORDS * 4);
	const uint8_t *hist_src = NULL; /* device: the end of the open linked frame's output so far */
	dbuf pack = {0, 0, 0};
	double t_read = 0, t_dec = 0, t_pack = 0, t_back = 0, t_write = 0, t_chk = 0, t0;
	size_t nbatch = 0, npack = 0, nblocks = 0, seg_blocks = 0, seg_segs = 0, seg_serial = 0;

	/* GPUMT_LZ4_RUN_PAR: 1 = the blocks of a linked run side by side (gpumt_lz4_decompress_blocks_par), 0 = one wave per
	 * run; unset or any other value: PL_PAR_DEFAULT, as profiles/plain_lz4_blocks.txt decided it.  The call keeps an origin
	 * plane of two bytes per byte of the batch's output inside the device boundary; where the device cannot give it, or
	 * the boundary has no such call, the batch decodes with the serial call, same bytes and verdicts. */
	const char *par_env = getenv("GPUMT_LZ4_RUN_PAR");
	const int par_set = par_env && (par_env[0] == '0' || par_env[0] == '1') && !par_env[1];
	__typeof__(gpumt_lz4_decompress_blocks) *const decode_blocks =
		gpumt_lz4_decompress_blocks_par && (par_set ? par_env[0] == '1' : PL_PAR_DEFAULT) ? gpumt_lz4_decompress_blocks_par
												      : gpumt_lz4_decompress_blocks;
	/* GPUMT_LZ4_BLOCK_SEG=1 (nothing else): every batch with gpumt_lz4_decompress_blocks_seg, big blocks in segments side by
	 * side, linked runs included, so it wins over GPUMT_LZ4_RUN_PAR; same bytes and verdicts, the same fall-backs */
	const char *seg_env = getenv("GPUMT_LZ4_BLOCK_SEG");
	const int seg_on = gpumt_lz4_decompress_blocks_seg && seg_env && seg_env[0] == '1' && !seg_env[1];

	memset(&fr, 0, sizeof fr);
	if (!gpumt_lz4_decompress_blocks || !gpumt_lz4_pack_runs || !gpumt_xxh32_carry || !gpumt_memcpy_d2d) {
		err = MTP(ERROR)(compression_library); /* a device boundary without the block-level calls */
		goto out;
	}
	if (!raw || !segs || !d_states) {
		err = MTP(ERROR)(memory_allocation);
		goto out;
	}
	memcpy(raw, first, nfirst);
	MT_PLAIN_ENTER(ctx, nfirst);
	while (!err && !done) {
		const int b = batch & 1;
		struct dslot *s = &ctx->s[b];
		const size_t want_ahead = need > BATCH_BYTES ? need : BATCH_BYTES;
		size_t jp, in_bytes = 0, out_bytes = 0, nblk = 0, nrun = 0, nseg = 0, perr = 0, hist = 0;
		int cur = -1; /* the segment of the frame the walker is in, once this batch holds something of it */
		gpumt_lz4_block *blocks;
		gpumt_lz4_run *runs;

		/* ---- read: the reference's request sizes (lz4-mt_decompress.c:462-476), until a batch of input is buffered ---- */
		t0 = pl_now();
		while (!eof && n - ip < want_ahead) {
			MTP(Buffer) rb;
			int rv;
			if (ip && ip == n)
				n = ip = 0;
			if (n + req > cap) {
				if (ip >= req) { /* drop what is decoded instead of growing */
					memmove(raw, raw + ip, n - ip);
					n -= ip;
					ip = 0;
				} else {
					uint8_t *nr;
					cap = cap * 2 + req;
					nr = (uint8_t *)realloc(raw, cap);
					if (!nr) {
						err = MTP(ERROR)(memory_allocation);
						goto out;
					}
					raw = nr;
				}
			}
			rb.buf = raw + n;
			rb.size = req;
			rb.allocated = req;
			rv = io->fn_read(io->arg_read, &rb);
			if (rv != 0) {
				err = mt_error(rv);
				goto out;
			}
			if (rb.size == 0) {
				eof = 1;
				break;
			}
			n += rb.size;
			ctx->insize += rb.size;
		}
		t_read += pl_now() - t0;

		/* ---- the slot's buffers: its last batch's checksum jobs are done with them ---- */
		t0 = pl_now();
		err = pl_settle(ctx, g, b, pend);
		t_chk += pl_now() - t0;
		if (err)
			break;
		if (dbuf_want(g, &s->meta, PL_META_BYTES, 1, 1) ||
		    dbuf_want(g, &s->in, (n - ip) + 512, 1, 1)) { /* the block bodies of a batch are part of what is buffered */
			err = MTP(ERROR)(memory_allocation);
			break;
		}
		blocks = PL_AT(gpumt_lz4_block, &s->meta, 0, PL_OFF_BLOCKS);
		runs = PL_AT(gpumt_lz4_run, &s->meta, 0, PL_OFF_RUNS);

		/* ---- walk: everything that is complete in raw[ip..n) and fits the batch ---- */
		need = 0;
		for (jp = ip;;) {
			const size_t avail = n - jp;
			const uint8_t *p = raw + jp;
			size_t want = 0; /* bytes the item at p needs, when they are not all there */
			if (skip_left) { /* inside a skippable frame */
				const size_t k = skip_left < avail ? (size_t)skip_left : avail;
				jp += k;
				skip_left -= k;
				if (skip_left)
					want = 1;
				else
					continue;
			} else if (!fr.open) {
				if (avail == 0 && eof) {
					done = 1;
					break;
				}
				if (avail < 4) {
					want = 4;
				} else if ((rd32(p) & 0xFFFFFFF0u) == MT_MAGIC_SKIPPABLE) {
					if (avail < 8) {
						want = 8;
					} else {
						skip_left = rd32(p + 4);
						jp += 8;
						continue;
					}
				} else if (rd32(p) == MT_FRAME_MAGIC) {
					if (avail < 7) {
						want = 7;
					} else {
						const unsigned flg = p[4], bd = p[5], bsid = (bd >> 4) & 7;
						const size_t hdr = 7 + ((flg & 8) ? 8 : 0) + ((flg & 1) ? 4 : 0); /* a dictionary id is skipped */
						if ((flg >> 6) != 1 || (flg & 2) || (bd & 0x8F) || bsid < 4) {
							perr = plain_bad_frame(); /* version, reserved bits, block size id */
							break;
						}
						if (avail < hdr) {
							want = hdr;
						} else {
							if (p[hdr - 1] != ((pl_xxh32_short(p + 4, hdr - 5) >> 8) & 0xFF)) {
								MT_ERRCODE = GPUMT_ST_BAD_FRAME;
								perr = plain_bad_frame();
								break;
							}
							if (nseg == PL_MAXB)
								break; /* the batch's segment table is full: the header is read again with the next batch */
							memset(&fr, 0, sizeof fr);
							fr.open = 1;
							fr.indep = (flg >> 5) & 1;
							fr.bchk = (flg >> 4) & 1;
							fr.has_csize = (flg >> 3) & 1;
							fr.cchk = (flg >> 2) & 1;
							fr.blkmax = 1u << (8 + 2 * bsid);
							fr.csize = fr.has_csize ? rd64(p + 6) : 0;
							jp += hdr;
							cur = (int)nseg++;
							memset(&segs[cur], 0, sizeof segs[cur]);
							segs[cur].first = 1;
							segs[cur].run0 = (uint32_t)nrun;
							continue;
						}
					}
				} else {
					perr = plain_bad_frame(); /* bytes that are no frame */
					break;
				}
			} else if (avail < 4) {
				want = 4;
			} else {
				const uint32_t bh = rd32(p), bsz = bh & 0x7FFFFFFFu;
				const int stored = (int)(bh >> 31);
				if (cur < 0) { /* the frame came from the batch before */
					if (nseg == PL_MAXB)
						break;
					cur = (int)nseg++;
					memset(&segs[cur], 0, sizeof segs[cur]);
					segs[cur].run0 = (uint32_t)nrun;
					segs[cur].before = fr.produced;
				}
				if (bh == 0) { /* end mark (+ content checksum) */
					const size_t tot = 4 + (fr.cchk ? 4u : 0u);
					if (avail < tot) {
						want = tot;
					} else {
						segs[cur].last = 1;
						segs[cur].cchk = fr.cchk;
						segs[cur].expect = fr.cchk ? rd32(p + 4) : 0;
						segs[cur].has_csize = fr.has_csize;
						segs[cur].csize = fr.csize;
						fr.open = 0;
						cur = -1;
						jp += tot;
						continue;
					}
				} else if (bsz > fr.blkmax) {
					MT_ERRCODE = GPUMT_ST_BAD_BLOCK;
					perr = MTP(ERROR)(compression_library);
					break;
				} else {
					const size_t tot = 4 + (size_t)bsz + (fr.bchk ? 4u : 0u);
					/* what the block can decode to: 255:1 is the format's maximum expansion */
					const uint32_t bcap = stored ? bsz : (bsz > fr.blkmax / 255 ? fr.blkmax : 255 * bsz);
					if (avail < tot) {
						want = tot;
					} else {
						gpumt_lz4_block *B;
						gpumt_lz4_run *R;
						if (nblk && (nblk == PL_MAXB || in_bytes + bsz > BATCH_BYTES || out_bytes + bcap > out_budget))
							break; /* the batch is full */
						B = &blocks[nblk];
						B->src_off = in_bytes;
						B->src_len = bsz;
						B->flags = (stored ? GPUMT_LZ4B_STORED : 0) | (fr.bchk ? GPUMT_LZ4B_CHECKSUM : 0);
						B->blkmax = fr.blkmax;
						B->checksum = fr.bchk ? rd32(p + 4 + bsz) : 0;
						memcpy((uint8_t *)s->in.h + in_bytes, p + 4, bsz);
						if (fr.indep || !segs[cur].nrun) {
							R = &runs[nrun++];
							memset(R, 0, sizeof *R);
							R->first = (uint32_t)nblk;
							R->low = out_bytes;
							if (!fr.indep && segs[cur].before) {
								/* a linked frame goes on: its last 64 KiB in front (the first thing of this batch) */
								hist = segs[cur].before < PL_HIST ? (size_t)segs[cur].before : PL_HIST;
								out_bytes += hist;
							}
							R->out_off = out_bytes;
							segs[cur].nrun++;
						} else {
							R = &runs[nrun - 1];
						}
						R->count++;
						R->out_cap += bcap;
						out_bytes += bcap;
						in_bytes += bsz;
						nblk++;
						jp += tot;
						continue;
					}
				}
			}
			/* the item at p is not complete */
			if (eof) {
				perr = plain_bad_frame(); /* truncated */
			} else {
				need = want;
				if (skip_left)
					need = 1;
			}
			break;
		}
		ip = jp;

		/* ---- decode what the walk collected ---- */
		if (nseg) {
			const size_t data0 = nrun ? (size_t)runs[0].out_off : 0;
			uint32_t *run_len = PL_AT(uint32_t, &s->meta, 0, PL_OFF_RUNLEN);
			uint32_t *status = PL_AT(uint32_t, &s->meta, 0, PL_OFF_STATUS);
			gpumt_xxh32_job *jobs = PL_AT(gpumt_xxh32_job, &s->meta, 0, PL_OFF_JOBS);
			size_t total = 0, njobs = 0;
			int contiguous = 1, rc = 0;
			const uint8_t *d_data;
			nbatch++;
			nblocks += nblk;
			if (nrun) {
				t0 = pl_now();
				if (dbuf_want(g, &s->out, out_bytes + 64, 1, 1)) {
					err = MTP(ERROR)(memory_allocation);
					break;
				}
				rc |= gpumt_memcpy_h2d(g, s->in.d, s->in.h, in_bytes, 0);
				rc |= gpumt_memcpy_h2d(g, PL_AT(void, &s->meta, 1, PL_OFF_BLOCKS), blocks, nblk * sizeof *blocks, 0);
				rc |= gpumt_memcpy_h2d(g, PL_AT(void, &s->meta, 1, PL_OFF_RUNS), runs, nrun * sizeof *runs, 0);
				if (hist) {
					if (!hist_src) {
						err = MTP(ERROR)(compression_library);
						break;
					}
					rc |= gpumt_memcpy_d2d(g, s->out.d, hist_src - hist, hist, 0);
				}
				if (seg_on) {
					rc |= gpumt_lz4_decompress_blocks_seg(
						g, s->in.d, in_bytes, PL_AT(gpumt_lz4_block, &s->meta, 1, PL_OFF_BLOCKS), nblk,
						PL_AT(gpumt_lz4_run, &s->meta, 1, PL_OFF_RUNS), nrun, s->out.d, out_bytes,
						PL_AT(uint32_t, &s->meta, 1, PL_OFF_BLKLEN), PL_AT(uint32_t, &s->meta, 1, PL_OFF_RUNLEN),
						PL_AT(uint32_t, &s->meta, 1, PL_OFF_STATUS), PL_AT(uint32_t, &s->meta, 1, PL_OFF_BLKSEG), 0);
					if (ctx->gpus.trace)
						rc |= gpumt_memcpy_d2h(g, PL_AT(void, &s->meta, 0, PL_OFF_BLKSEG),
								       PL_AT(void, &s->meta, 1, PL_OFF_BLKSEG), nblk * 4, 0);
				} else {
					rc |= decode_blocks(g, s->in.d, in_bytes, PL_AT(gpumt_lz4_block, &s->meta, 1, PL_OFF_BLOCKS), nblk,
							    PL_AT(gpumt_lz4_run, &s->meta, 1, PL_OFF_RUNS), nrun, s->out.d, out_bytes,
							    PL_AT(uint32_t, &s->meta, 1, PL_OFF_BLKLEN), PL_AT(uint32_t, &s->meta, 1, PL_OFF_RUNLEN),
							    PL_AT(uint32_t, &s->meta, 1, PL_OFF_STATUS), 0);
				}
				rc |= gpumt_memcpy_d2h(g, run_len, PL_AT(void, &s->meta, 1, PL_OFF_RUNLEN), nrun * 4, 0);
				rc |= gpumt_memcpy_d2h(g, status, PL_AT(void, &s->meta, 1, PL_OFF_STATUS), nrun * 4, 0);
				rc |= gpumt_stream_sync(g, 0);
				t_dec += pl_now() - t0;
				if (rc) {
					err = MTP(ERROR)(compression_library);
					break;
				}
				if (seg_on && ctx->gpus.trace) {
					const uint32_t *bs = PL_AT(uint32_t, &s->meta, 0, PL_OFF_BLKSEG);
					for (size_t k = 0; k < nblk; k++) {
						seg_blocks++;
						seg_segs += bs[k];
						seg_serial += bs[k] == 0;
					}
				}
				for (size_t r = 0; r < nrun; r++) {
					if (status[r] != GPUMT_ST_OK) {
						MT_ERRCODE = status[r];
						err = MTP(ERROR)(compression_library);
						break;
					}
					if (runs[r].out_off != data0 + total)
						contiguous = 0; /* a slot before this one came out short */
					total += run_len[r];
				}
				if (err)
					break;
			}
			/* the slots of independent blocks -> one piece, unless every one came out full (all but a frame's last do) */
			d_data = (const uint8_t *)s->out.d + data0;
			if (!contiguous) {
				t0 = pl_now();
				if (pack_busy) { /* the last batch's checksum jobs still read the pack area */
					rc |= gpumt_stream_sync(g, PL_XS);
					pack_busy = 0;
				}
				if (dbuf_want(g, &pack, total + 64, 0, 1)) {
					err = MTP(ERROR)(memory_allocation);
					break;
				}
				rc |= gpumt_lz4_pack_runs(g, s->out.d, out_bytes, PL_AT(gpumt_lz4_run, &s->meta, 1, PL_OFF_RUNS),
							  PL_AT(uint32_t, &s->meta, 1, PL_OFF_RUNLEN), nrun, pack.d, total,
							  PL_AT(uint64_t, &s->meta, 1, PL_OFF_PACKOFF), 0);
				d_data = (const uint8_t *)pack.d;
				npack++;
				t_pack += pl_now() - t0;
			}
			/* ---- per frame: the size it states, its content checksum (carried over the batches), its history ---- */
			{
				size_t at = 0, r = 0;
				for (size_t k = 0; k < nseg && !err; k++) {
					struct pl_seg *sg = &segs[k];
					size_t len = 0;
					for (; r < sg->run0 + sg->nrun; r++)
						len += run_len[r];
					if (sg->last && sg->has_csize && sg->csize != sg->before + len) {
						MT_ERRCODE = GPUMT_ST_SIZE_MISMATCH;
						err = MTP(ERROR)(compression_library);
						break;
					}
					if (sg->last ? sg->cchk : fr.cchk) {
						gpumt_xxh32_job *J = &jobs[njobs++];
						J->off = at;
						J->len = (uint32_t)len;
						J->flags = (sg->first ? GPUMT_XXH_RESET : GPUMT_XXH_IN(xs)) |
							   (sg->last ? GPUMT_XXH_FINAL | GPUMT_XXH_VERIFY : GPUMT_XXH_OUT(xs ^ 1));
						J->expect = sg->expect;
						J->reserved = 0;
						if (!sg->last)
							xs ^= 1;
					}
					if (!sg->last) { /* the frame goes on with the next batch */
						fr.produced = sg->before + len;
						hist_src = !fr.indep && sg->nrun ? (const uint8_t *)s->out.d + runs[sg->run0].out_off + len : hist_src;
					}
					at += len;
				}
				if (err)
					break;
			}
			if (njobs) {
				rc |= gpumt_stream_wait(g, PL_XS, 0);
				rc |= gpumt_memcpy_h2d(g, PL_AT(void, &s->meta, 1, PL_OFF_JOBS), jobs, njobs * sizeof *jobs, PL_XS);
				rc |= gpumt_xxh32_carry(g, total ? (const void *)d_data : (const void *)s->in.d, total,
							PL_AT(gpumt_xxh32_job, &s->meta, 1, PL_OFF_JOBS), njobs, d_states,
							PL_AT(uint32_t, &s->meta, 1, PL_OFF_DIGEST),
							PL_AT(uint32_t, &s->meta, 1, PL_OFF_VERDICT), PL_XS);
				rc |= gpumt_memcpy_d2h(g, PL_AT(void, &s->meta, 0, PL_OFF_VERDICT), PL_AT(void, &s->meta, 1, PL_OFF_VERDICT),
						       njobs * 4, PL_XS);
				rc |= gpumt_mark(g, b, PL_XS);
				pend[b] = njobs;
				pack_busy = !contiguous;
			}
			if (total) {
				t0 = pl_now();
				rc |= gpumt_memcpy_d2h(g, s->out.h, d_data, total, 0);
				rc |= gpumt_stream_sync(g, 0);
				t_back += pl_now() - t0;
			}
			if (rc) {
				err = MTP(ERROR)(compression_library);
				break;
			}
			t0 = pl_now();
			err = plain_write(ctx, io, (const uint8_t *)s->out.h, total);
			t_write += pl_now() - t0;
			if (nrun)
				batch++; /* (a batch without runs leaves the slots as they are: the open linked frame's history stays in the other one) */
		}
		if (!err)
			err = perr;
	}
	/* the checksum jobs still under way, oldest first */
	t0 = pl_now();
	for (int k = 0; k < 2; k++) {
		const size_t e = pl_settle(ctx, g, (batch + k) & 1, pend);
		if (!err)
			err = e;
	}
	t_chk += pl_now() - t0;
out:
	mt_gpus_sync(&ctx->gpus);
	if (ctx->gpus.trace)
		fprintf(stderr,
			"[lz4mt plain] %zu batches, %zu blocks, %zu packed; read %.1f ms, h2d+decode %.1f ms, pack %.1f ms, d2h %.1f ms, "
			"write %.1f ms, waiting for the content checksum %.1f ms\n",
			nbatch, nblocks, npack, 1e3 * t_read, 1e3 * t_dec, 1e3 * t_pack, 1e3 * t_back, 1e3 * t_write, 1e3 * t_chk);
	if (ctx->gpus.trace)
		fprintf(stderr, "[lz4mt plain par] linked runs %s\n",
			decode_blocks != gpumt_lz4_decompress_blocks ? "block-parallel" : "one wave each");
	if (ctx->gpus.trace && seg_on)
		fprintf(stderr, "[lz4mt plain seg] %zu blocks in %zu segments, %zu serial\n", seg_blocks, seg_segs, seg_serial);
	dbuf_free(g, &pack);
	if (d_states)
		gpumt_free(g, d_states);
	free(segs);
	free(raw);
	return err;
}
