/*
 * mt_zstd_plain.inc -- the plain .zst path of ZSTDCB_decompressDCtx: a stream that starts with a zstd frame instead of a
 * skippable record (files of the zstd tool and of libzstd callers).  The reference decodes it on one thread with streaming
 * ZSTD_decompressStream (st_decompress, lib/zstd-mt_decompress.c:552-687), at any size and in constant memory.  Here the
 * unit of work is the block run, as the block is in mt_lz4_plain.inc: a state machine walks the bytes read so far (frame
 * header, 3-byte block headers, the optional content checksum; skippable frames in between are dropped), every block that
 * is complete in the buffer goes into the batch's block table, and the consecutive blocks of one frame that a batch holds
 * are one run, decoded by one wave (gpumt_zstd_decompress_blocks).  Whole frames inside a batch are runs of their own and
 * decode side by side.  A frame that goes on into the next batch leaves its decoder state (repeat offsets, Huffman and FSE
 * tables) in a carry slot on the device, and the last min(bytes so far, window) bytes of its output are copied in front
 * of the next batch's output, device to device, for the matches that reach back.  So host memory is about two batches of
 * input plus one block, device memory two batches of output plus a window, whatever the frame's size, and a frame's size
 * has no limit (its totals are 64-bit here).
 * Under GPUMT_ZSTD_RUN_PRE=1, in front of the runs the device decodes the Huffman literals and the FSE sequences of all blocks of the batch side by side
 * (gpumt_zstd_decompress_blocks_pre), which leaves a run's wave the table building and the sequence execution.  That takes
 * GPUMT_ZSTD_PRE_SCRATCH(128 KiB) = 384 KiB of device scratch per block of the largest batch so far -- three times a
 * batch's output for a frame of full blocks, more where blocks are smaller, up to 3 GiB for 8192 blocks -- inside the device
 * boundary; where the device cannot give it, or the boundary
 * has no such call, the batch decodes with the serial call, same bytes and verdicts.
 * Every plain frame takes this path, not only those larger than a batch: one walker and one decoder for plain input.
 * The content checksum is one serial XXH64 chain over the frame; its state lives on the device, is continued batch by
 * batch (gpumt_xxh64_carry) on stream ZP_XS and is settled when the batch's buffers are taken again, so it runs under
 * the next batch's read, decode and write.  One batch at a time otherwise: read, decode, write on the calling thread.
 * As with the reference's streaming decoder, output of earlier batches (and of a batch whose checksum later turns out
 * wrong) may have been written when an error surfaces; the return value is what counts.
 * Included by zstdmt_engine.c behind mt_records12.inc (the context, plain_write).  Plain C, no HIP header.
 */
#include <time.h>

/* The device calls that only this path uses are weak references here, as in mt_lz4_plain.inc: a stand-in for the device
 * boundary that does not provide them (the plain-C one of the ThreadSanitizer runs, which only ever feeds records) still
 * links, and this path then fails with compression_library -- an error, not another way to decode. */
extern __typeof__(gpumt_zstd_decompress_blocks) gpumt_zstd_decompress_blocks __attribute__((weak));
extern __typeof__(gpumt_zstd_decompress_blocks_pre) gpumt_zstd_decompress_blocks_pre __attribute__((weak));
extern __typeof__(gpumt_zstd_decompress_blocks_par) gpumt_zstd_decompress_blocks_par __attribute__((weak));
extern __typeof__(gpumt_xxh64_carry) gpumt_xxh64_carry __attribute__((weak));
extern __typeof__(gpumt_memcpy_d2d) gpumt_memcpy_d2d __attribute__((weak));

#define ZP_MAXB BATCH_MAXREC /* blocks, runs, frame segments of one batch */
#define ZP_XS 3 /* the stream of the carried content checksum */
#define ZP_WINDOW_MAX ((uint64_t)1 << 27) /* ZSTD_WINDOWLOG_LIMIT_DEFAULT: what the reference's streaming decoder takes */

/* the tables of a batch in the slot's `meta` buffer (pinned mirror and device copy alike) */
#define ZP_OFF_BLOCKS 0
#define ZP_OFF_RUNS (ZP_OFF_BLOCKS + sizeof(gpumt_zstd_block) * ZP_MAXB)
#define ZP_OFF_JOBS (ZP_OFF_RUNS + sizeof(gpumt_zstd_run) * ZP_MAXB)
#define ZP_OFF_RUNLEN (ZP_OFF_JOBS + sizeof(gpumt_xxh32_job) * ZP_MAXB)
#define ZP_OFF_STATUS (ZP_OFF_RUNLEN + 4 * ZP_MAXB)
#define ZP_OFF_DIGEST (ZP_OFF_STATUS + 4 * ZP_MAXB)
#define ZP_OFF_VERDICT (ZP_OFF_DIGEST + 4 * ZP_MAXB)
#define ZP_OFF_MARK (ZP_OFF_VERDICT + 4 * ZP_MAXB) /* the pre-pass's verdict per block: read back under GPUMT_TRACE only */
#define ZP_META_BYTES (ZP_OFF_MARK + 4 * ZP_MAXB + 64)
#define ZP_AT(type, meta, dev, off) ((type *)((uint8_t *)((dev) ? (meta)->d : (meta)->h) + (off)))

struct zp_frame { /* the frame the walker is inside of */
	int open, cchk, has_csize;
	int started;     /* a run of it has been queued: the next one continues the carry */
	int blocks_done; /* its last block is walked, the content checksum is what is missing */
	int slot;        /* its carry slot on the device */
	uint32_t block_max;
	uint64_t window, csize, produced; /* produced: content bytes of the batches before this one */
};

struct zp_seg { /* the part of one frame a batch holds */
	int run; /* its run in this batch, -1: none (header or checksum only) */
	int first, last, cchk, has_csize;
	uint32_t expect;
	uint64_t csize, before; /* before: the frame's content ahead of this batch */
};

static double zp_now(void)
{
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* the verdicts of the checksum jobs slot b left behind: waited for before the slot's buffers are taken again */
static size_t zp_settle(MTP(DCtx) *ctx, gpumt_ctx *g, int b, size_t *pend)
{
	size_t err = 0;
	if (!pend[b])
		return 0;
	if (gpumt_mark_sync(g, b))
		err = MTP(ERROR)(compression_library);
	for (size_t j = 0; j < pend[b] && !err; j++) {
		const uint32_t v = ZP_AT(uint32_t, &ctx->s[b].meta, 0, ZP_OFF_VERDICT)[j];
		if (v != GPUMT_ST_OK) {
			MT_ERRCODE = v;
			err = MTP(ERROR)(compression_library);
		}
	}
	pend[b] = 0;
	return err;
}

static size_t zp_fail(uint32_t code)
{
	MT_ERRCODE = code;
	return MTP(ERROR)(compression_library);
}

/* first[0..nfirst) came with the sniff; at_eof: the sniff already hit the end of the input */
static size_t plain_decompress(MTP(DCtx) *ctx, MTP(RdWr_t) *io, const uint8_t *first, size_t nfirst, int at_eof)
{
	const size_t req = MT_PLAIN_REQUEST(ctx);
	/* output a batch may decode to: as the input budget allows at 4:1, at most 1 GiB (positions inside a run are 32 bits) */
	const size_t out_budget = 4 * BATCH_BYTES < ((size_t)1 << 30) ? 4 * BATCH_BYTES : (size_t)1 << 30;
	size_t cap = req, n = nfirst, ip = 0, err = 0, need = 4, pend[2] = {0, 0};
	uint8_t *raw = (uint8_t *)malloc(cap);
	int eof = at_eof, first_read = 1, batch = 0, xs = 0, cslot = 0, done = 0;
	uint64_t skip_left = 0;
	struct zp_frame fr;
	struct zp_seg *segs = (struct zp_seg *)malloc(sizeof(struct zp_seg) * ZP_MAXB);
	gpumt_ctx *g = mt_gpu_of(&ctx->gpus, 0);
	uint32_t *d_states = NULL;
	void *d_carry = NULL;
	const uint8_t *hist_src = NULL; /* device: the end of the open frame's output so far */
	double t_read = 0, t_dec = 0, t_hist = 0, t_back = 0, t_write = 0, t_chk = 0, t0;
	size_t nbatch = 0, nblocks = 0, nruns = 0, npre_seq = 0, npre_lit = 0;

	/* The entropy stage is asked for with GPUMT_ZSTD_RUN_PRE=1 and otherwise off: its rate against the serial call has not
	 * been measured on a device (profiles/plain_zst_blocks.txt), and it takes three launches and its scratch per batch. */
	const char *pre_env = getenv("GPUMT_ZSTD_RUN_PRE");
	const int use_pre = gpumt_zstd_decompress_blocks_pre && pre_env && pre_env[0] == '1' && !pre_env[1];
	/* The block-parallel execute stage behind it (gpumt_zstd_decompress_blocks_par) likewise, under GPUMT_ZSTD_RUN_PAR=1
	 * only: whether it becomes the default is decided from profiles/plain_zst_blocks.txt. */
	const char *par_env = getenv("GPUMT_ZSTD_RUN_PAR");
	const int use_par = gpumt_zstd_decompress_blocks_par && par_env && par_env[0] == '1' && !par_env[1];

	memset(&fr, 0, sizeof fr);
	if (!gpumt_zstd_decompress_blocks || !gpumt_xxh64_carry || !gpumt_memcpy_d2d) {
		err = MTP(ERROR)(compression_library); /* a device boundary without the block-level calls */
		goto out;
	}
	d_states = (uint32_t *)gpumt_malloc(g, 2 * GPUMT_XXH64_STATE_WORDS * 4);
	d_carry = gpumt_malloc(g, 2 * GPUMT_ZSTD_CARRY_BYTES);
	if (!raw || !segs || !d_states || !d_carry) {
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
		gpumt_zstd_block *blocks;
		gpumt_zstd_run *runs;

		/* ---- read: the reference's request sizes (the first one fills the first buffer behind the sniffed bytes,
		 * zstd-mt_decompress.c:590-609), until a batch of input is buffered ---- */
		t0 = zp_now();
		while (!eof && n - ip < want_ahead) {
			MTP(Buffer) rb;
			int rv;
			const size_t want = first_read ? req - nfirst : req;
			if (ip && ip == n)
				n = ip = 0;
			if (n + want > cap) {
				if (ip >= want) { /* drop what is decoded instead of growing */
					memmove(raw, raw + ip, n - ip);
					n -= ip;
					ip = 0;
				} else {
					uint8_t *nr;
					cap = cap * 2 + want;
					nr = (uint8_t *)realloc(raw, cap);
					if (!nr) {
						err = MTP(ERROR)(memory_allocation);
						goto out;
					}
					raw = nr;
				}
			}
			rb.buf = raw + n;
			rb.size = want;
			rb.allocated = want;
			rv = io->fn_read(io->arg_read, &rb);
			if (rv != 0) {
				err = mt_error(rv);
				goto out;
			}
			first_read = 0;
			if (rb.size == 0) {
				eof = 1;
				break;
			}
			n += rb.size;
			ctx->insize += rb.size;
		}
		t_read += zp_now() - t0;

		/* ---- the slot's buffers: its last batch's checksum jobs are done with them ---- */
		t0 = zp_now();
		err = zp_settle(ctx, g, b, pend);
		t_chk += zp_now() - t0;
		if (err)
			break;
		if (dbuf_want(g, &s->meta, ZP_META_BYTES, 1, 1) ||
		    dbuf_want(g, &s->in, (n - ip) + 512, 1, 1)) { /* the blocks of a batch are part of what is buffered */
			err = MTP(ERROR)(memory_allocation);
			break;
		}
		blocks = ZP_AT(gpumt_zstd_block, &s->meta, 0, ZP_OFF_BLOCKS);
		runs = ZP_AT(gpumt_zstd_run, &s->meta, 0, ZP_OFF_RUNS);

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
				} else if (rd32(p) != MT_FRAME_MAGIC) {
					perr = plain_bad_frame(); /* bytes that are no frame */
					break;
				} else if (avail < 6) {
					want = 6;
				} else { /* frame header, RFC 8878 3.1.1.1 */
					const unsigned fhd = p[4], fcs = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
					const unsigned did_len = did == 3 ? 4 : did, fcs_len = fcs == 0 ? single : 1u << fcs;
					const size_t hdr = 5 + (1 - single) + did_len + fcs_len;
					if (fhd & 8) {
						perr = plain_bad_frame(); /* reserved bit */
						break;
					}
					if (avail < hdr) {
						want = hdr;
					} else {
						size_t hp = 5;
						uint64_t window = 0, content = 0, id = 0;
						if (!single) {
							const unsigned wd = p[hp++];
							const uint64_t base = 1ull << (10 + (wd >> 3));
							window = base + (base >> 3) * (wd & 7);
						}
						for (unsigned k = 0; k < did_len; k++)
							id |= (uint64_t)p[hp + k] << (8 * k);
						hp += did_len;
						for (unsigned k = 0; k < fcs_len; k++)
							content |= (uint64_t)p[hp + k] << (8 * k);
						if (fcs == 1)
							content += 256;
						if (single)
							window = content;
						if (id) {
							perr = zp_fail(GPUMT_ST_UNSUPPORTED); /* no dictionaries */
							break;
						}
						if (window > ZP_WINDOW_MAX) {
							perr = plain_bad_frame(); /* frameParameter_windowTooLarge in the reference */
							break;
						}
						if (nseg == ZP_MAXB)
							break; /* the batch's segment table is full: the header is read again with the next batch */
						memset(&fr, 0, sizeof fr);
						fr.open = 1;
						fr.cchk = (fhd >> 2) & 1;
						fr.has_csize = fcs_len != 0;
						fr.csize = content;
						fr.window = window;
						fr.block_max = window < 131072 ? (uint32_t)window : 131072u;
						jp += hdr;
						cur = (int)nseg++;
						memset(&segs[cur], 0, sizeof segs[cur]);
						segs[cur].first = 1;
						segs[cur].run = -1;
						continue;
					}
				}
			} else {
				if (cur < 0) { /* the frame came from the batch before */
					if (nseg == ZP_MAXB)
						break;
					cur = (int)nseg++;
					memset(&segs[cur], 0, sizeof segs[cur]);
					segs[cur].run = -1;
					segs[cur].before = fr.produced;
				}
				if (fr.blocks_done) { /* the content checksum, and the frame is complete */
					const size_t tot = fr.cchk ? 4u : 0u;
					if (avail < tot) {
						want = tot;
					} else {
						segs[cur].last = 1;
						segs[cur].cchk = fr.cchk;
						segs[cur].expect = fr.cchk ? rd32(p) : 0;
						segs[cur].has_csize = fr.has_csize;
						segs[cur].csize = fr.csize;
						fr.open = 0;
						cur = -1;
						jp += tot;
						continue;
					}
				} else if (avail < 3) {
					want = 3;
				} else {
					const uint32_t bh = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
					const uint32_t last = bh & 1, type = (bh >> 1) & 3, bsize = bh >> 3;
					const size_t tot = 3 + (type == 1 ? 1u : (size_t)bsize);
					/* what the block decodes to at most: its own size when raw or RLE */
					const uint32_t bcap = type == 2 ? fr.block_max : bsize;
					if (type == 3 || bsize > fr.block_max) {
						perr = zp_fail(GPUMT_ST_BAD_BLOCK); /* reserved type, above Block_Maximum_Size */
						break;
					}
					if (avail < tot) {
						want = tot;
					} else {
						gpumt_zstd_block *B;
						gpumt_zstd_run *R;
						if (nblk && (nblk == ZP_MAXB || in_bytes + tot > BATCH_BYTES || out_bytes + bcap > out_budget))
							break; /* the batch is full */
						B = &blocks[nblk];
						B->src_off = in_bytes;
						B->src_len = (uint32_t)tot;
						B->block_max = fr.block_max;
						memcpy((uint8_t *)s->in.h + in_bytes, p, tot);
						if (segs[cur].run < 0) {
							segs[cur].run = (int)nrun;
							R = &runs[nrun++];
							memset(R, 0, sizeof *R);
							R->first = (uint32_t)nblk;
							if (fr.started) {
								/* the frame goes on: its last window of output in front (the first thing of this batch) */
								hist = fr.produced < fr.window ? (size_t)fr.produced : (size_t)fr.window;
								out_bytes += hist;
								R->hist = (uint32_t)hist;
								R->carry = (uint32_t)fr.slot;
							} else {
								R->flags = GPUMT_ZRUN_FIRST;
							}
							R->out_off = out_bytes;
							fr.started = 1;
						} else {
							R = &runs[nrun - 1];
						}
						R->count++;
						R->out_cap += bcap;
						out_bytes += bcap;
						in_bytes += tot;
						nblk++;
						jp += tot;
						if (last) {
							fr.blocks_done = 1;
							R->flags |= GPUMT_ZRUN_LAST;
						}
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
		/* a frame that starts in this batch and goes on: its state leaves in the carry slot the batch's other runs do not read */
		if (nrun && (runs[nrun - 1].flags & (GPUMT_ZRUN_FIRST | GPUMT_ZRUN_LAST)) == GPUMT_ZRUN_FIRST) {
			fr.slot = cslot ^= 1;
			runs[nrun - 1].carry = (uint32_t)fr.slot;
		}

		/* ---- decode what the walk collected ---- */
		if (nseg) {
			uint32_t *run_len = ZP_AT(uint32_t, &s->meta, 0, ZP_OFF_RUNLEN);
			uint32_t *status = ZP_AT(uint32_t, &s->meta, 0, ZP_OFF_STATUS);
			gpumt_xxh32_job *jobs = ZP_AT(gpumt_xxh32_job, &s->meta, 0, ZP_OFF_JOBS);
			size_t total = 0, njobs = 0;
			int rc = 0;
			nbatch++;
			nblocks += nblk;
			nruns += nrun;
			if (nrun) {
				if (dbuf_want(g, &s->out, out_bytes + 64, 1, 1)) {
					err = MTP(ERROR)(memory_allocation);
					break;
				}
				if (hist) {
					t0 = zp_now();
					if (!hist_src) {
						err = MTP(ERROR)(compression_library);
						break;
					}
					rc |= gpumt_memcpy_d2d(g, s->out.d, hist_src - hist, hist, 0);
					if (ctx->gpus.trace)
						rc |= gpumt_stream_sync(g, 0); /* so that the stage's time is its own */
					t_hist += zp_now() - t0;
				}
				t0 = zp_now();
				rc |= gpumt_memcpy_h2d(g, s->in.d, s->in.h, in_bytes, 0);
				rc |= gpumt_memcpy_h2d(g, ZP_AT(void, &s->meta, 1, ZP_OFF_BLOCKS), blocks, nblk * sizeof *blocks, 0);
				rc |= gpumt_memcpy_h2d(g, ZP_AT(void, &s->meta, 1, ZP_OFF_RUNS), runs, nrun * sizeof *runs, 0);
				if (use_par) {
					rc |= gpumt_zstd_decompress_blocks_par(g, s->in.d, in_bytes,
									       ZP_AT(gpumt_zstd_block, &s->meta, 1, ZP_OFF_BLOCKS), nblk,
									       ZP_AT(gpumt_zstd_run, &s->meta, 1, ZP_OFF_RUNS), nrun, s->out.d,
									       out_bytes, d_carry, ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_RUNLEN),
									       ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_STATUS),
									       ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_MARK), NULL, 0);
					if (ctx->gpus.trace)
						rc |= gpumt_memcpy_d2h(g, ZP_AT(void, &s->meta, 0, ZP_OFF_MARK), ZP_AT(void, &s->meta, 1, ZP_OFF_MARK),
								       nblk * 4, 0);
				} else if (use_pre) {
					rc |= gpumt_zstd_decompress_blocks_pre(g, s->in.d, in_bytes,
									       ZP_AT(gpumt_zstd_block, &s->meta, 1, ZP_OFF_BLOCKS), nblk,
									       ZP_AT(gpumt_zstd_run, &s->meta, 1, ZP_OFF_RUNS), nrun, s->out.d,
									       out_bytes, d_carry, ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_RUNLEN),
									       ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_STATUS),
									       ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_MARK), 0);
					if (ctx->gpus.trace)
						rc |= gpumt_memcpy_d2h(g, ZP_AT(void, &s->meta, 0, ZP_OFF_MARK), ZP_AT(void, &s->meta, 1, ZP_OFF_MARK),
								       nblk * 4, 0);
				} else {
					rc |= gpumt_zstd_decompress_blocks(g, s->in.d, in_bytes,
									   ZP_AT(gpumt_zstd_block, &s->meta, 1, ZP_OFF_BLOCKS), nblk,
									   ZP_AT(gpumt_zstd_run, &s->meta, 1, ZP_OFF_RUNS), nrun, s->out.d, out_bytes,
									   d_carry, ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_RUNLEN),
									   ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_STATUS), 0);
				}
				rc |= gpumt_memcpy_d2h(g, run_len, ZP_AT(void, &s->meta, 1, ZP_OFF_RUNLEN), nrun * 4, 0);
				rc |= gpumt_memcpy_d2h(g, status, ZP_AT(void, &s->meta, 1, ZP_OFF_STATUS), nrun * 4, 0);
				rc |= gpumt_stream_sync(g, 0);
				t_dec += zp_now() - t0;
				if (rc) {
					err = MTP(ERROR)(compression_library);
					break;
				}
				if (ctx->gpus.trace && (use_pre || use_par))
					for (size_t k = 0; k < nblk; k++) {
						const uint32_t mk = ZP_AT(uint32_t, &s->meta, 0, ZP_OFF_MARK)[k];
						npre_seq += mk & 1;
						npre_lit += (mk >> 1) & 1;
					}
				for (size_t r = 0; r < nrun && !err; r++)
					if (status[r] != GPUMT_ST_OK)
						err = zp_fail(status[r]);
				if (err)
					break;
			}
			/* ---- per frame: the size it states, its content checksum (carried over the batches), its history ---- */
			for (size_t k = 0; k < nseg && !err; k++) {
				struct zp_seg *sg = &segs[k];
				const size_t len = sg->run >= 0 ? run_len[sg->run] : 0;
				const size_t at = sg->run >= 0 ? (size_t)runs[sg->run].out_off : 0;
				if (sg->last && sg->has_csize && sg->csize != sg->before + len) {
					err = zp_fail(GPUMT_ST_SIZE_MISMATCH);
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
					if (sg->run >= 0)
						hist_src = (const uint8_t *)s->out.d + at + len;
				}
				total += len;
			}
			if (err)
				break;
			if (njobs) {
				rc |= gpumt_stream_wait(g, ZP_XS, 0);
				rc |= gpumt_memcpy_h2d(g, ZP_AT(void, &s->meta, 1, ZP_OFF_JOBS), jobs, njobs * sizeof *jobs, ZP_XS);
				rc |= gpumt_xxh64_carry(g, nrun ? (const void *)s->out.d : (const void *)s->in.d, nrun ? out_bytes : 0,
							ZP_AT(gpumt_xxh32_job, &s->meta, 1, ZP_OFF_JOBS), njobs, d_states,
							ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_DIGEST),
							ZP_AT(uint32_t, &s->meta, 1, ZP_OFF_VERDICT), ZP_XS);
				rc |= gpumt_memcpy_d2h(g, ZP_AT(void, &s->meta, 0, ZP_OFF_VERDICT), ZP_AT(void, &s->meta, 1, ZP_OFF_VERDICT),
						       njobs * 4, ZP_XS);
				rc |= gpumt_mark(g, b, ZP_XS);
				pend[b] = njobs;
			}
			if (total) {
				/* the runs' bytes, in order, to one piece of pinned memory: neighbours that came out full go in one copy */
				size_t to = 0;
				t0 = zp_now();
				for (size_t r = 0; r < nrun;) {
					const size_t from = (size_t)runs[r].out_off;
					size_t span = run_len[r];
					for (r++; r < nrun && runs[r].out_off == from + span; r++)
						span += run_len[r];
					if (span)
						rc |= gpumt_memcpy_d2h(g, (uint8_t *)s->out.h + to, (const uint8_t *)s->out.d + from, span, 0);
					to += span;
				}
				rc |= gpumt_stream_sync(g, 0);
				t_back += zp_now() - t0;
			}
			if (rc) {
				err = MTP(ERROR)(compression_library);
				break;
			}
			t0 = zp_now();
			err = plain_write(ctx, io, (const uint8_t *)s->out.h, total);
			t_write += zp_now() - t0;
			if (nrun)
				batch++; /* (a batch without runs leaves the slots as they are: the open frame's history stays in the other one) */
		}
		if (!err)
			err = perr;
	}
	/* the checksum jobs still under way, oldest first */
	t0 = zp_now();
	for (int k = 0; k < 2; k++) {
		const size_t e = zp_settle(ctx, g, (batch + k) & 1, pend);
		if (!err)
			err = e;
	}
	t_chk += zp_now() - t0;
out:
	mt_gpus_sync(&ctx->gpus);
	if (ctx->gpus.trace)
		fprintf(stderr,
			"[zstdmt plain] %zu batches, %zu blocks, %zu runs; read %.1f ms, history %.1f ms, h2d+decode %.1f ms, d2h %.1f ms, "
			"write %.1f ms, waiting for the content checksum %.1f ms\n",
			nbatch, nblocks, nruns, 1e3 * t_read, 1e3 * t_hist, 1e3 * t_dec, 1e3 * t_back, 1e3 * t_write, 1e3 * t_chk);
	if (ctx->gpus.trace)
		fprintf(stderr, "[zstdmt plain pre] %zu blocks: sequences of %zu and literals of %zu decoded ahead\n", nblocks,
			npre_seq, npre_lit);
	if (d_carry)
		gpumt_free(g, d_carry);
	if (d_states)
		gpumt_free(g, d_states);
	free(segs);
	free(raw);
	return err;
}
