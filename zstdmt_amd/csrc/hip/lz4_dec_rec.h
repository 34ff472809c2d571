/*
 * lz4_dec_rec.h -- from a batch of lz4-mt records to the block and run tables of the block calls
 * (gpumt_lz4_decompress_batch_par); included by lz4_dec.hip behind lz4_dec_seg.h, and by gpumt.hip for the record layout
 * and the slice rule alone (LREC_HOST_ONLY).  The LZ4 twin of zstd_dec_rec.h.
 *
 * A record of several linked blocks is one serial chain for the record decoders (one wave per record in the copy stage,
 * one wave for the whole record in zmt_lz4_dec_serial).  gpumt_lz4_decompress_blocks_par / _seg decode such a chain side by
 * side, but want a table of blocks and runs; the records are device memory, so the tables are made here.  One lane per
 * record throughout, no wave waits on another:
 *
 *   count    reads the 12-byte header and the LZ4F frame header and hops from block header to block header to the end mark:
 *            the block count, where the first block header is, blkmax, the content size, the checksum flags, one past the
 *            end mark, and `eligible`.  It decides no verdict: whatever it does not like is not eligible, and the record
 *            decoders judge it.
 *   (host)   cuts the batch into slices of consecutive records (lrec_next_slice), each one call of the block stages.
 *   scan     one workgroup per slice: for every eligible record its run and its first block in the slice's tables.
 *   table    walks the frame again and writes the block entries and the run.
 *   finish   keeps a record whose run came back clean with the stated content size.  A kept record gets ST_REC_KEPT in
 *            the scratch status words, which the record decoders read as their "kept" array and pass by.
 *   merge    d_status = OK for a kept record that the record decoders passed by, else what they said.
 */
#ifndef ZMT_LZ4_DEC_REC_H
#define ZMT_LZ4_DEC_REC_H

#ifndef ST_REC_KEPT
#define ST_REC_KEPT 102u /* internal, scratch status only: the block stages decoded the record */
#endif
#define LREC_ELIGIBLE 1u
#define LREC_CCHECK 2u /* 4 bytes of content checksum behind the end mark */
#define LREC_BCHECK 4u /* 4 bytes of block checksum behind every block */
#define LREC_MAX_RUNS 4096u
#define LREC_MAX_STREAM 0xFFFFFFF0ull
#define LREC_MAX_BLOCKS 65536u /* a record of more blocks stays with the record decoders */
#define LREC_MAX_CONTENT 0xFFFE0000u /* gpumt_lz4_run.out_cap */

struct LRec { /* what count leaves per record; the host reads a copy */
	u64 rec_off, out_off;
	u64 content; /* the frame's content size, ~0 = none stated */
	u32 rec_len, out_len;
	u32 nblk, flags;
	u32 first;  /* the first block header, from the start of the record */
	u32 blkmax; /* from BD: 64 KiB .. 4 MiB */
	u32 end;    /* one past the end mark, from the start of the record */
	u32 pad;
};

struct LRecSlice {
	size_t a, b;        /* records [a, b): a and b - 1 are eligible */
	u32 nrun, nblk;     /* eligible records and their blocks */
	u64 in_lo, in_hi;   /* what they span of d_stream (in_lo rounded down to 256, so alignments stay what they were) */
	u64 out_lo, out_hi; /* ... and of d_out, likewise */
};

/* The next slice from record `at` on: at most LREC_MAX_RUNS eligible records, max_blocks blocks and LREC_MAX_STREAM stream
 * bytes; a record of more than max_blocks blocks is a slice of its own.  -> false when no eligible record is left. */
static inline bool lrec_next_slice(const LRec *recs, size_t nrec, size_t at, u32 max_blocks, LRecSlice *S)
{
	size_t i = at;
	while (i < nrec && !(recs[i].flags & LREC_ELIGIBLE))
		i++;
	if (i == nrec)
		return false;
	S->a = S->b = i;
	S->nrun = S->nblk = 0;
	S->in_lo = S->out_lo = ~0ull;
	S->in_hi = S->out_hi = 0;
	for (; i < nrec; i++) {
		const LRec &R = recs[i];
		if (!(R.flags & LREC_ELIGIBLE))
			continue;
		const u64 ilo = (R.rec_off & ~255ull) < S->in_lo ? (R.rec_off & ~255ull) : S->in_lo;
		const u64 ihi = R.rec_off + R.rec_len > S->in_hi ? R.rec_off + R.rec_len : S->in_hi;
		if (S->nrun && (S->nrun == LREC_MAX_RUNS || S->nblk + R.nblk > max_blocks || ihi - ilo > LREC_MAX_STREAM))
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

#ifndef LREC_HOST_ONLY

/* seg_bytes: 0 = the blocks are the parts (gpumt_lz4_decompress_blocks_par); else the segment of
 * gpumt_lz4_decompress_blocks_seg, and a record has max(blocks, ceil(content / seg_bytes)) parts */
extern "C" __global__ void __launch_bounds__(256)
zmt_lz4_rec_count_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const u64 *__restrict__ rec_off,
			 const u32 *__restrict__ rec_len, u32 nrec, const u64 *__restrict__ out_off,
			 const u32 *__restrict__ out_len, u64 out_bytes, u32 min_blocks, u32 seg_bytes, LRec *__restrict__ recs)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nrec)
		return;
	LRec R;
	R.rec_off = rec_off[i];
	R.out_off = out_off[i];
	R.content = ~0ull;
	R.rec_len = rec_len[i];
	R.out_len = out_len[i];
	R.nblk = R.flags = R.first = R.blkmax = R.end = R.pad = 0;
	do {
		const u32 rlen = R.rec_len;
		/* a record or an output range that leaves the batch, or that the run tables cannot express */
		if (R.rec_off > stream_bytes || rlen > stream_bytes - R.rec_off || rlen > 0xFFFFFE00u || R.out_off > out_bytes ||
		    R.out_len > out_bytes - R.out_off || R.out_len > LREC_MAX_CONTENT)
			break;
		const u8 *r = stream + R.rec_off;
		if (rlen < 12 + 7 || ld32u(r) != ZMT_SKIP_MAGIC || ld32u(r + 4) != 4 || ld32u(r + 8) != rlen - 12 ||
		    ld32u(r + 12) != ZMT_LZ4F_MAGIC)
			break;
		const u8 *f = r + 12;
		const u32 flen = rlen - 12;
		const u32 flg = f[4], bd = f[5];
		/* version, reserved bits, block maximum id (parse_frame_header); independent blocks and frames without a content
		 * size are not this stage's */
		if ((flg >> 6) != 1 || (flg & 0x02) || (bd & 0x8F) || (bd >> 4) < 4 || (flg & 0x20) || !(flg & 0x08))
			break;
		const u32 hdr = 7 + 8 + ((flg & 0x01) ? 4u : 0u);
		if (flen < hdr)
			break;
		{
			u8 d[14];
			for (u32 k = 0; k < hdr - 5; k++)
				d[k] = f[4 + k];
			if (f[hdr - 1] != ((xxh32_short(d, hdr - 5) >> 8) & 0xFF))
				break;
		}
		R.content = (u64)ld32u(f + 6) | (u64)ld32u(f + 10) << 32;
		R.blkmax = 1u << (8 + 2 * (bd >> 4));
		R.first = 12 + hdr;
		if (flg & 0x10)
			R.flags |= LREC_BCHECK;
		if (flg & 0x04)
			R.flags |= LREC_CCHECK;
		if (R.content != R.out_len || R.content == 0)
			break;
		const u32 bc = (flg & 0x10) ? 4u : 0u;
		u32 p = hdr, n = 0;
		bool closed = false;
		while (flen - p >= 4 && n <= LREC_MAX_BLOCKS) {
			const u32 bh = ld32u(f + p);
			p += 4;
			if (bh == 0) {
				closed = true;
				break;
			}
			const u32 bsz = bh & 0x7FFFFFFFu;
			if (bsz > R.blkmax || flen - p < bsz || flen - p - bsz < bc)
				break; /* a block above the maximum, or one that would leave the record */
			p += bsz + bc;
			n++;
		}
		R.nblk = n;
		R.end = 12 + p;
		if (!closed || n == 0 || n > LREC_MAX_BLOCKS || flen - p != ((flg & 0x04) ? 4u : 0u))
			break;
		u32 parts = n;
		if (seg_bytes) {
			const u32 by_size = (u32)((R.content + seg_bytes - 1) / seg_bytes);
			parts = by_size > n ? by_size : n;
		}
		if (parts >= min_blocks)
			R.flags |= LREC_ELIGIBLE;
	} while (0);
	recs[i] = R;
}

/* per eligible record of a slice of n records: rrun = the eligible records in front of it, rfirst = their blocks */
extern "C" __global__ void __launch_bounds__(256)
zmt_lz4_rec_scan_kernel(const LRec *__restrict__ recs, u32 n, u32 *__restrict__ rfirst, u32 *__restrict__ rrun)
{
	__shared__ u32 pb[256], pr[256];
	const u32 t = threadIdx.x;
	const u32 per = (n + 255) / 256;
	const u32 lo = t * per < n ? t * per : n;
	const u32 hi = lo + per < n ? lo + per : n;
	u32 sb = 0, sr = 0;
	for (u32 i = lo; i < hi; i++)
		if (recs[i].flags & LREC_ELIGIBLE) {
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
		if (recs[i].flags & LREC_ELIGIBLE) {
			b += recs[i].nblk;
			r++;
		}
	}
}

/* the slice's tables: offsets count from in_lo / out_lo, where the slice's d_stream and d_out start */
extern "C" __global__ void __launch_bounds__(256)
zmt_lz4_rec_table_kernel(const u8 *__restrict__ stream, const LRec *__restrict__ recs, u32 n, const u32 *__restrict__ rfirst,
			 const u32 *__restrict__ rrun, u64 in_lo, u64 out_lo, u32 nblk, u32 nrun, Lz4Block *__restrict__ blocks,
			 Lz4Run *__restrict__ runs)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const LRec R = recs[i];
	if (!(R.flags & LREC_ELIGIBLE))
		return;
	const u32 first = rfirst[i], run = rrun[i];
	if (run >= nrun || first > nblk || R.nblk > nblk - first)
		return; /* (cannot be: the host sized the tables from the same counts) */
	const u8 *r = stream + R.rec_off;
	const u32 bc = (R.flags & LREC_BCHECK) ? 4u : 0u;
	u32 p = R.first;
	for (u32 k = 0; k < R.nblk; k++) {
		/* (count walked the same bytes: every header and body lies inside the record) */
		const u32 bh = ld32u(r + p);
		const u32 bsz = bh & 0x7FFFFFFFu;
		Lz4Block B;
		B.src_off = R.rec_off - in_lo + p + 4;
		B.src_len = bsz;
		B.flags = ((bh & 0x80000000u) ? LZ4B_STORED : 0u) | (bc ? LZ4B_CHECKSUM : 0u);
		B.blkmax = R.blkmax;
		B.checksum = bc ? ld32u(r + p + 4 + bsz) : 0u;
		blocks[first + k] = B;
		p += 4 + bsz + bc;
	}
	Lz4Run U;
	U.low = U.out_off = R.out_off - out_lo; /* a frame's first block has no history */
	U.out_cap = (u32)R.content;
	U.first = first;
	U.count = R.nblk;
	U.reserved = 0;
	runs[run] = U;
}

extern "C" __global__ void __launch_bounds__(256)
zmt_lz4_rec_finish_kernel(const u8 *__restrict__ stream, const LRec *__restrict__ recs, u32 n, const u32 *__restrict__ rrun,
			  u32 nrun, const u32 *__restrict__ run_len, const u32 *__restrict__ run_status,
			  u32 *__restrict__ out_len, u32 *__restrict__ rec_par, u32 *__restrict__ sstatus,
			  u32 *__restrict__ chk_expect, u32 *__restrict__ chk_valid)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const LRec R = recs[i];
	if (!(R.flags & LREC_ELIGIBLE))
		return;
	const u32 run = rrun[i];
	if (run >= nrun || run_status[run] != ST_OK)
		return;
	if (R.content != run_len[run])
		return;
	out_len[i] = (u32)R.content;
	if (R.flags & LREC_CCHECK) {
		chk_expect[i] = ld32u(stream + R.rec_off + R.end);
		chk_valid[i] = 1;
	}
	if (rec_par)
		rec_par[i] = R.nblk;
	sstatus[i] = ST_REC_KEPT;
}

/* The record decoders acknowledge a record they passed by with ST_REC_KEPT in d_status.  One they decoded after all has
 * their verdict and their bytes, and is not counted as kept */
extern "C" __global__ void __launch_bounds__(256)
zmt_lz4_rec_merge_kernel(const u32 *__restrict__ sstatus, u32 nrec, u32 *__restrict__ status, u32 *__restrict__ rec_par)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nrec || sstatus[i] != ST_REC_KEPT)
		return;
	if (status[i] == ST_REC_KEPT)
		status[i] = ST_OK;
	else if (rec_par)
		rec_par[i] = 0;
}

#endif /* LREC_HOST_ONLY */
#endif
