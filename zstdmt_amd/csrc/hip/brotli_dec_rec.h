/*
 * brotli_dec_rec.h -- from a batch of brotli-mt records to a table of spans (gpumt_brotli_decompress_batch_par); included by
 * brotli_dec4.hip, whose zmt_brotli_dec4_span_kernel decodes the table, by brotli_enc.hip for the index layout, and by
 * gpumt.hip for the record layout and the slice rule alone (BREC_HOST_ONLY).  The brotli twin of lz4_dec_rec.h.
 *
 * A brotli stream is one serial chain: a meta-block starts at a bit position that only the decode of everything before it
 * finds.  The streams of gpumt_brotli_compress_batch_index say where they can be cut.  Every 128 KiB block is a meta-block
 * of its own, padded to a byte boundary, with no match source outside the block and no use of a distance from before it; and
 * in front of the closing 0x03 byte lies one metadata meta-block (RFC 7932 section 9.2, skipped by every decoder) whose
 * payload is the index:
 *
 *   header   byte-aligned: ISLAST 0, MNIBBLES 11, reserved 0, MSKIPBYTES nb, MSKIPLEN - 1 in nb bytes, two zero bits:
 *            nb + 1 bytes, the least nb that holds the length
 *   body     n x { u32 comp_bytes, u32 out_bytes }, then { u32 n, u32 BREC_MAGIC }, little endian
 *
 * Span k is stream bytes [sum comp_bytes[<k], + comp_bytes[k]) and decodes to out_bytes[k] bytes; span 0 starts at stream
 * byte 0 with the WBITS bits.  The index is found from the record's end: the last byte 0x03, the 8 trailer bytes in front
 * of it, the body of 8 n + 8 bytes, the header.
 *
 * The index is a hint and is never trusted.  One lane per record in the stages here, no wave waits on another:
 *
 *   plan     finds the index and checks it: the magic, min_spans <= n <= 65536, no zero entry, sum comp_bytes + header +
 *            body + 1 == the record's length, the bytes at sum comp_bytes are exactly that header, sum out_bytes <= the
 *            record's capacity, a WBITS that brotli-mt allows.  It decides no verdict: a record that fails is not eligible.
 *   (host)   cuts the batch into slices of consecutive records (brec_next_slice), each one launch of the execute stage.
 *   scan     one workgroup per slice: for every eligible record its first entry in the slice's span table.
 *   table    writes the entries: stream range, output offset, out_bytes, WBITS.
 *   execute  zmt_brotli_dec4_span_kernel (brotli_dec4.hip): the dec4 scheme with a span as the unit.  A group refuses -- any
 *            status but ST_OK -- what dec4 hands over (context modelling, block switching, a large distance alphabet), an
 *            ISLAST bit inside the span, a meta-block that does not end where the span ends, a decoded length other than
 *            out_bytes, a copy whose source lies before the span's first output byte (which covers every static dictionary
 *            reference: such a distance is larger still) and, in a span behind the first, a distance code that reads a
 *            ring entry the span did not write.
 *   finish   keeps a record all of whose spans came back ST_OK: out_len = sum out_bytes, status ST_OK, rec_par = 1.  Every
 *            other record keeps BREC_TODO in its status word, and the record decoders (zmt_brotli_dec4_wanted_kernel, the
 *            general kernel) decode and judge exactly those: the verdicts are the serial call's by construction.
 *
 * Why a kept record is the serial decode, byte for byte.  The spans tile the stream from byte 0 to the index block (the
 * sum check).  Each span was decoded from a byte boundary to its end exactly, ending on a meta-block boundary -- so the
 * serial decoder, which reaches byte 0 of span 0 in the same state, reaches every span's first bit at a meta-block boundary
 * too, by induction.  At such a boundary a decoder without context modelling carries three things: the output so far, the
 * distance ring and the window size.  No span read output from before its start or a ring entry from before its start (the
 * refusals), and WBITS is the stream's own, so each span decoded what the serial decoder decodes there, to out_bytes[k]
 * bytes at the offset the sum of the earlier ones gives.  Behind the last span the plan verified a well-formed metadata
 * meta-block that ends one byte before the record's end, and that last byte is 0x03 -- ISLAST, ISLASTEMPTY, zero padding:
 * the serial decoder skips the one, stops at the other and reports sum out_bytes, which the plan checked against the capacity.
 */
#ifndef ZMT_BROTLI_DEC_REC_H
#define ZMT_BROTLI_DEC_REC_H

#define BREC_MAGIC 0x58495242u /* "BRIX" */
#define BREC_MAX_SPANS 65536u  /* a record of more spans gets no index / stays with the record decoders */
#define BREC_TODO 103u         /* internal status: the record decoders decode the record (B4_HANDOFF is 102) */
#define BREC_ELIGIBLE 1u       /* BRec.flags; WBITS << 8 */
#define BREC_SLICE_SPANS (1u << 20)

/* bytes of the index block of n spans: header + body */
#define BREC_BODY(n) (8u * (n) + 8u)
#define BREC_NB(n) (BREC_BODY(n) - 1u < 256u ? 1u : BREC_BODY(n) - 1u < 65536u ? 2u : 3u)
#define BREC_INDEX_BYTES(n) (BREC_NB(n) + 1u + BREC_BODY(n))
/* the header as one little-endian value of BREC_NB(n) + 1 bytes */
#define BREC_HEADER(n) (0x06u | BREC_NB(n) << 4 | (BREC_BODY(n) - 1u) << 6)

struct BRec { /* what plan leaves per record; the host reads a copy */
	u64 rec_off, out_off;
	u32 rec_len, out_sum; /* out_sum: what the spans decode to together */
	u32 nspan, flags;
};

#define B4_SPAN_FIRST 1u /* B4Span.flags: the span opens the stream (WBITS header, the RFC's initial distance ring) */
struct B4Span {
	u64 src, out;         /* from d_stream / d_out */
	u32 src_len, out_len; /* stream bytes, and the bytes they must decode to */
	u32 rec, flags;       /* B4_SPAN_FIRST | WBITS << 8 */
};

struct BRecSlice {
	size_t a, b; /* records [a, b) */
	u32 nspan;   /* spans of their eligible records */
};

/* The next slice from record `at` on: eligible records of at most max_spans spans together (one record may have more: it
 * is a slice of its own).  -> false when no eligible record is left. */
static inline bool brec_next_slice(const BRec *recs, size_t nrec, size_t at, u32 max_spans, BRecSlice *S)
{
	size_t i = at;
	while (i < nrec && !(recs[i].flags & BREC_ELIGIBLE))
		i++;
	if (i == nrec)
		return false;
	S->a = S->b = i;
	S->nspan = 0;
	for (; i < nrec; i++) {
		if (!(recs[i].flags & BREC_ELIGIBLE))
			continue;
		if (S->nspan && S->nspan + recs[i].nspan > max_spans)
			break;
		S->nspan += recs[i].nspan;
		S->b = i + 1;
	}
	return true;
}

#ifndef BREC_HOST_ONLY

extern "C" __global__ void __launch_bounds__(256)
zmt_brotli_rec_plan_kernel(const u8 *__restrict__ stream, const u64 *__restrict__ rec_off, const u32 *__restrict__ rec_len,
			   u32 nrec, const u64 *__restrict__ out_off, const u32 *__restrict__ out_cap, u32 min_spans,
			   BRec *__restrict__ recs)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nrec)
		return;
	BRec R;
	R.rec_off = rec_off[i];
	R.out_off = out_off[i];
	R.rec_len = rec_len[i];
	R.out_sum = R.nspan = R.flags = 0;
	do {
		const u32 rlen = R.rec_len;
		const u8 *r = stream + R.rec_off;
		/* two spans of a byte, the smallest index block and the last byte; 32-bit bit positions in the execute stage */
		if (rlen < 2u + BREC_INDEX_BYTES(2u) + 1u || rlen >= (1u << 28) || r[rlen - 1] != 0x03)
			break;
		const u32 n = ld32u(r + rlen - 9);
		if (ld32u(r + rlen - 5) != BREC_MAGIC || n < 2u || n < min_spans || n > BREC_MAX_SPANS)
			break;
		const u32 nb = BREC_NB(n), idx_bytes = BREC_INDEX_BYTES(n);
		if (rlen - 1u < idx_bytes + n)
			break;
		const u32 at = rlen - 1u - idx_bytes; /* where the index block must start: sum comp_bytes */
		u32 hv = 0;
		for (u32 k = 0; k <= nb; k++)
			hv |= (u32)r[at + k] << (8 * k);
		if (hv != BREC_HEADER(n))
			break;
		const u8 *e = r + at + nb + 1u;
		u64 csum = 0, osum = 0;
		bool zero = false;
		for (u32 k = 0; k < n; k++) {
			const u32 c = ld32u(e + 8 * k), o = ld32u(e + 8 * k + 4);
			zero |= c == 0 || o == 0;
			csum += c;
			osum += o;
		}
		if (zero || csum != at || osum > out_cap[i])
			break;
		/* WBITS (RFC 7932 9.1), as zmt_brotli_dec4_kernel reads it; the large-window form is not brotli-mt's */
		const u32 b0 = r[0];
		u32 wbits = 16;
		if (b0 & 1u) {
			const u32 v = (b0 >> 1) & 7u, w = (b0 >> 4) & 7u;
			if (!v && w == 1u)
				break;
			wbits = v ? 17u + v : w ? 8u + w : 17u;
		}
		R.nspan = n;
		R.out_sum = (u32)osum;
		R.flags = BREC_ELIGIBLE | wbits << 8;
	} while (0);
	recs[i] = R;
}

/* per record of a slice of n records: ufirst = the spans of the eligible records in front of it */
extern "C" __global__ void __launch_bounds__(256)
zmt_brotli_rec_scan_kernel(const BRec *__restrict__ recs, u32 n, u32 *__restrict__ ufirst)
{
	__shared__ u32 ps[256];
	const u32 t = threadIdx.x;
	const u32 per = (n + 255) / 256;
	const u32 lo = t * per < n ? t * per : n;
	const u32 hi = lo + per < n ? lo + per : n;
	u32 sum = 0;
	for (u32 i = lo; i < hi; i++)
		if (recs[i].flags & BREC_ELIGIBLE)
			sum += recs[i].nspan;
	ps[t] = sum;
	__syncthreads();
	for (u32 d = 1; d < 256; d <<= 1) {
		const u32 v = t >= d ? ps[t - d] : 0;
		__syncthreads();
		ps[t] += v;
		__syncthreads();
	}
	u32 u = ps[t] - sum;
	for (u32 i = lo; i < hi; i++) {
		ufirst[i] = u;
		if (recs[i].flags & BREC_ELIGIBLE)
			u += recs[i].nspan;
	}
}

extern "C" __global__ void __launch_bounds__(256)
zmt_brotli_rec_table_kernel(const u8 *__restrict__ stream, const BRec *__restrict__ recs, u32 n, u32 rec0,
			    const u32 *__restrict__ ufirst, u32 nspan, B4Span *__restrict__ spans)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const BRec R = recs[i];
	if (!(R.flags & BREC_ELIGIBLE))
		return;
	const u32 first = ufirst[i];
	if (first > nspan || R.nspan > nspan - first)
		return; /* (cannot be: the host sized the table from the same counts) */
	/* (plan read the same bytes: the entries lie inside the record and their sums fit) */
	const u8 *e = stream + R.rec_off + R.rec_len - 1u - BREC_BODY(R.nspan);
	u64 src = R.rec_off, out = R.out_off;
	for (u32 k = 0; k < R.nspan; k++) {
		B4Span U;
		U.src = src;
		U.out = out;
		U.src_len = ld32u(e + 8 * k);
		U.out_len = ld32u(e + 8 * k + 4);
		U.rec = rec0 + i;
		U.flags = (k ? 0u : B4_SPAN_FIRST) | (R.flags & ~0xFFu);
		spans[first + k] = U;
		src += U.src_len;
		out += U.out_len;
	}
}

extern "C" __global__ void __launch_bounds__(256)
zmt_brotli_rec_finish_kernel(const BRec *__restrict__ recs, u32 n, const u32 *__restrict__ ufirst, u32 nspan,
			     const B4Span *__restrict__ spans, const u32 *__restrict__ span_status, u32 *__restrict__ out_len,
			     u32 *__restrict__ status, u32 *__restrict__ rec_par)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const BRec R = recs[i];
	if (!(R.flags & BREC_ELIGIBLE))
		return;
	const u32 first = ufirst[i];
	if (first > nspan || R.nspan > nspan - first)
		return;
	u32 sum = 0; /* (what the spans decoded: plan checked it against the capacity) */
	for (u32 k = 0; k < R.nspan; k++) {
		if (span_status[first + k] != ST_OK)
			return;
		sum += spans[first + k].out_len;
	}
	out_len[i] = sum;
	status[i] = ST_OK;
	if (rec_par)
		rec_par[i] = 1;
}

#endif /* BREC_HOST_ONLY */
#endif
