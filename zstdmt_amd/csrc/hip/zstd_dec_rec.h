/*
 * zstd_dec_rec.h -- from a batch of zstd-mt records to the block and run tables of the block-parallel calls
 * (gpumt_zstd_decompress_batch_par); included by zstd_dec.hip behind zstd_dec_par.h, and by gpumt.hip for the record
 * layout and the slice rule alone (ZREC_HOST_ONLY).
 *
 * A record of several blocks is one serial chain for the record decoders (one wave per frame).  The block calls decode
 * such a chain side by side, but want a table of blocks and runs; the records are device memory, so the tables are made
 * here.  One lane per record throughout, no wave waits on another:
 *
 *   count    reads the 12-byte header and the frame header and hops from block header to block header: the block count,
 *            where the first block starts, block_max, the content size, whether a checksum follows, and `eligible`.  It
 *            decides no verdict: whatever it does not like is not eligible, and the record decoders judge it.
 *   (host)   cuts the batch into slices of consecutive records (zrec_next_slice), each one call of the block stages.
 *   scan     one workgroup per slice: for every eligible record its run and its first block in the slice's tables.
 *   table    walks the frame again and writes the block entries and the run.
 *   finish   keeps a record whose run came back clean: the length is the stated content size, and behind the last block
 *            lie the 4 checksum bytes the descriptor promises and nothing else.  A kept record gets ST_REC_KEPT in the
 *            scratch copy of the status array, so the record decoders pass it by; every other record is theirs.
 *   merge    d_status = OK for a kept record, else what the record decoders said.
 */
#ifndef ZMT_ZSTD_DEC_REC_H
#define ZMT_ZSTD_DEC_REC_H

#define ST_REC_KEPT 102u /* internal, scratch status only: the block stages decoded the record */
#define ZREC_ELIGIBLE 1u
#define ZREC_CHECKSUM 2u
#define ZREC_MAX_RUNS 4096u /* the block calls' own limit for their stages */
#define ZREC_MAX_STREAM 0xFFFFFFF0ull
#define ZREC_MAX_BLOCKS 65536u /* a record of more blocks stays with the record decoders */

struct ZRec { /* what count leaves per record; the host reads a copy */
	u64 rec_off, out_off;
	u64 content; /* Frame_Content_Size, ~0 = none stated */
	u32 rec_len, out_len;
	u32 nblk, flags;
	u32 first;     /* the first block header, from the start of the record */
	u32 block_max; /* min(window, 128 KiB) */
	u32 end;       /* one past the last block, from the start of the record */
	u32 pad;
};

struct ZRecSlice {
	size_t a, b;       /* records [a, b): a and b - 1 are eligible */
	u32 nrun, nblk;    /* eligible records and their blocks */
	u64 in_lo, in_hi;  /* what they span of d_stream (in_lo rounded down to 256, so alignments stay what they were) */
	u64 out_lo, out_hi; /* ... and of d_out, likewise */
};

/* The next slice from record `at` on: at most ZREC_MAX_RUNS eligible records, max_blocks blocks and ZREC_MAX_STREAM stream
 * bytes; a record of more than max_blocks blocks is a slice of its own.  -> false when no eligible record is left. */
static inline bool zrec_next_slice(const ZRec *recs, size_t nrec, size_t at, u32 max_blocks, ZRecSlice *S)
{
	size_t i = at;
	while (i < nrec && !(recs[i].flags & ZREC_ELIGIBLE))
		i++;
	if (i == nrec)
		return false;
	S->a = S->b = i;
	S->nrun = S->nblk = 0;
	S->in_lo = S->out_lo = ~0ull;
	S->in_hi = S->out_hi = 0;
	for (; i < nrec; i++) {
		const ZRec &R = recs[i];
		if (!(R.flags & ZREC_ELIGIBLE))
			continue;
		const u64 ilo = (R.rec_off & ~255ull) < S->in_lo ? (R.rec_off & ~255ull) : S->in_lo;
		const u64 ihi = R.rec_off + R.rec_len > S->in_hi ? R.rec_off + R.rec_len : S->in_hi;
		if (S->nrun && (S->nrun == ZREC_MAX_RUNS || S->nblk + R.nblk > max_blocks || ihi - ilo > ZREC_MAX_STREAM))
			break;
		const u64 olo = R.out_off & ~255ull, ohi = R.out_off + R.out_len;
		S->in_lo = ilo;
		S->in_hi = ihi;
		S->out_lo = olo < S->out_lo ? olo : S->out_lo;
		S->out_hi = ohi > S->out_hi ? ohi : S->out_hi;
		S->nrun++;
		S->nblk += R.nblk;
		S->b = i + 1;
	}
	return true;
}

#ifndef ZREC_HOST_ONLY

/* the frame header of record R (RFC 8878 3.1.1), read by one lane -> where the first block starts (from the start of the
 * frame), 0 = not a frame this stage takes */
static __device__ __forceinline__ u32 zrec_frame_header(const u8 *f, u32 flen, u64 *content, u32 *block_max, u32 *has_chk)
{
	const u32 fhd = f[4], fcs = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
	const u32 fcs_len = fcs == 0 ? single : (1u << fcs);
	u32 hp = 5;
	u64 window = 0, c = ~0ull;
	/* reserved bit, a Dictionary_ID field (even one that says 0), a header that leaves the frame */
	if ((fhd & 8) || did || flen < 5 + (1 - single) + fcs_len)
		return 0;
	if (!single) {
		const u32 wd = f[hp++];
		const u64 base = 1ull << (10 + (wd >> 3));
		window = base + (base >> 3) * (wd & 7);
	}
	if (fcs_len) {
		c = 0;
		for (u32 k = 0; k < fcs_len; k++)
			c |= (u64)f[hp + k] << (8 * k);
		if (fcs == 1)
			c += 256;
	}
	hp += fcs_len;
	if (single)
		window = c;
	*content = c;
	*block_max = window < Z_BLOCK_MAX ? (u32)window : Z_BLOCK_MAX;
	*has_chk = (fhd >> 2) & 1;
	return hp;
}

extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_rec_count_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const u64 *__restrict__ rec_off,
			  const u32 *__restrict__ rec_len, u32 nrec, const u64 *__restrict__ out_off,
			  const u32 *__restrict__ out_len, u64 out_bytes, const u32 *__restrict__ status, u32 min_blocks,
			  ZRec *__restrict__ recs)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nrec)
		return;
	ZRec R;
	R.rec_off = rec_off[i];
	R.out_off = out_off[i];
	R.content = ~0ull;
	R.rec_len = rec_len[i];
	R.out_len = out_len[i];
	R.nblk = R.flags = R.first = R.block_max = R.end = R.pad = 0;
	do {
		const u32 rlen = R.rec_len;
		if (status[i] != ST_OK)
			break;
		/* a record or an output range that leaves the batch, or that the run tables cannot express */
		if (R.rec_off > stream_bytes || rlen > stream_bytes - R.rec_off || rlen > 0xFFFFFE00u || R.out_off > out_bytes ||
		    R.out_len > out_bytes - R.out_off || R.out_len > 0xFFFE0000u)
			break;
		const u8 *r = stream + R.rec_off;
		if (rlen < 12 + 6 || ld32u(r) != ZMT_SKIP_MAGIC || ld32u(r + 4) != 4 || ld32u(r + 8) != rlen - 12 ||
		    ld32u(r + 12) != ZMT_ZSTD_MAGIC)
			break;
		const u8 *f = r + 12;
		const u32 flen = rlen - 12;
		u32 has_chk = 0;
		u32 p = zrec_frame_header(f, flen, &R.content, &R.block_max, &has_chk);
		if (!p || (R.content != ~0ull && R.content != R.out_len))
			break;
		R.first = 12 + p;
		u32 n = 0;
		bool closed = false;
		while (flen - p >= 3) {
			const u32 bh = (u32)f[p] | (u32)f[p + 1] << 8 | (u32)f[p + 2] << 16;
			const u32 btype = (bh >> 1) & 3, body = btype == 1 ? 1u : bh >> 3;
			if (btype == 3 || flen - p - 3 < body)
				break; /* a block that would leave the record */
			p += 3 + body;
			n++;
			if (bh & 1) {
				closed = true;
				break;
			}
		}
		R.nblk = n;
		R.end = 12 + p;
		if (has_chk)
			R.flags |= ZREC_CHECKSUM;
		if (closed && n >= min_blocks && n <= ZREC_MAX_BLOCKS)
			R.flags |= ZREC_ELIGIBLE;
	} while (0);
	recs[i] = R;
}

/* per eligible record of a slice of n records: rrun = the eligible records in front of it, rfirst = their blocks */
extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_rec_scan_kernel(const ZRec *__restrict__ recs, u32 n, u32 *__restrict__ rfirst, u32 *__restrict__ rrun)
{
	__shared__ u32 pb[256], pr[256];
	const u32 t = threadIdx.x;
	const u32 per = (n + 255) / 256;
	const u32 lo = t * per < n ? t * per : n;
	const u32 hi = lo + per < n ? lo + per : n;
	u32 sb = 0, sr = 0;
	for (u32 i = lo; i < hi; i++)
		if (recs[i].flags & ZREC_ELIGIBLE) {
			sb += recs[i].nblk;
			sr++;
		}
	pb[t] = sb;
	pr[t] = sr;
	__syncthreads();
	for (u32 d = 1; d < 256; d <<= 1) {
		const u32 vb = t >= d ? pb[t - d] : 0, vr = t >= d ? pr[t - d] : 0;
		__syncthreads();
		pb[t] += vb;
		pr[t] += vr;
		__syncthreads();
	}
	u32 b = pb[t] - sb, r = pr[t] - sr;
	for (u32 i = lo; i < hi; i++) {
		rfirst[i] = b;
		rrun[i] = r;
		if (recs[i].flags & ZREC_ELIGIBLE) {
			b += recs[i].nblk;
			r++;
		}
	}
}

/* the slice's tables: offsets count from in_lo / out_lo, where the slice's d_stream and d_out start */
extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_rec_table_kernel(const u8 *__restrict__ stream, const ZRec *__restrict__ recs, u32 n, const u32 *__restrict__ rfirst,
			  const u32 *__restrict__ rrun, u64 in_lo, u64 out_lo, u32 nblk, u32 nrun, ZBlock *__restrict__ blocks,
			  ZRun *__restrict__ runs)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const ZRec R = recs[i];
	if (!(R.flags & ZREC_ELIGIBLE))
		return;
	const u32 first = rfirst[i], run = rrun[i];
	if (run >= nrun || first > nblk || R.nblk > nblk - first)
		return; /* (cannot be: the host sized the tables from the same counts) */
	const u8 *r = stream + R.rec_off;
	u32 p = R.first;
	for (u32 k = 0; k < R.nblk && R.rec_len - p >= 3; k++) {
		const u32 bh = (u32)r[p] | (u32)r[p + 1] << 8 | (u32)r[p + 2] << 16;
		const u32 body = ((bh >> 1) & 3) == 1 ? 1u : bh >> 3;
		ZBlock B;
		B.src_off = R.rec_off - in_lo + p;
		B.src_len = 3 + body;
		B.block_max = R.block_max;
		blocks[first + k] = B;
		p += 3 + body;
	}
	ZRun U;
	U.out_off = R.out_off - out_lo;
	U.out_cap = R.out_len;
	U.hist = 0;
	U.first = first;
	U.count = R.nblk;
	U.flags = ZR_FIRST | ZR_LAST;
	U.carry = 0;
	runs[run] = U;
}

extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_rec_finish_kernel(const u8 *__restrict__ stream, const ZRec *__restrict__ recs, u32 n, const u32 *__restrict__ rrun,
			   u32 nrun, const u32 *__restrict__ run_len, const u32 *__restrict__ run_status,
			   u32 *__restrict__ out_len, u32 *__restrict__ rec_par, u32 *__restrict__ sstatus,
			   u32 *__restrict__ chk_expect, u32 *__restrict__ chk_valid)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const ZRec R = recs[i];
	if (!(R.flags & ZREC_ELIGIBLE))
		return;
	const u32 run = rrun[i];
	if (run >= nrun || run_status[run] != ST_OK)
		return;
	const u32 len = run_len[run], chk = R.flags & ZREC_CHECKSUM ? 4u : 0u;
	if ((R.content != ~0ull && R.content != len) || R.rec_len - R.end != chk)
		return;
	if (R.content == ~0ull)
		out_len[i] = len;
	if (chk) {
		chk_expect[i] = ld32u(stream + R.rec_off + R.end);
		chk_valid[i] = 1;
	}
	if (rec_par)
		rec_par[i] = R.nblk;
	sstatus[i] = ST_REC_KEPT;
}

extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_rec_merge_kernel(const u32 *__restrict__ sstatus, u32 nrec, u32 *__restrict__ status)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nrec)
		return;
	const u32 s = sstatus[i];
	status[i] = s == ST_REC_KEPT ? (u32)ST_OK : s;
}

#endif /* ZREC_HOST_ONLY */
#endif
