/*
 * brotli_dec4.hip -- brotli stream decoder for gfx950, FOUR records per wave ("dec4").
 *
 * Replaces BrotliDecoderDecompress as called per record by the reference
 * (/root/reference/lib/brotli-mt_decompress.c:344-346) for the streams that make up BASELINE configs[4]: what
 * the reference's compressor writes at levels 0..4 -- meta-blocks with ONE block type per category, ONE literal
 * tree (no context modelling), ONE distance tree.  Every other stream (block switching, context maps, static
 * dictionary references) is handed to the general kernel (brotli_dec.hip) by status B4_HANDOFF, so the pair
 * decodes everything RFC 7932 allows.
 *
 * Why: a brotli stream is one serial bitstream, and brotli_dec.hip walks it in wave-uniform control flow -- one
 * record per wave, 70 % of its instructions on the scalar pipe, which the 16 waves of a CU saturate
 * (profiles/r03_sq_counters.json: 31 wave-instructions per output byte).  Here a wave runs FOUR streams side by
 * side, one per 16-lane group, in lockstep at the command level: one pass of the loop decodes one insert&copy
 * command of each of the four records, so every instruction of the command and distance decode serves four
 * commands, and the literal loop runs max(insert lengths) times instead of their sum.  All per-stream state is
 * "group-uniform" vector state (every lane of a group holds the same value); the canonical prefix decode of
 * brotli_dec.hip -- lane l of a tree's vector holds the left-aligned end of the code range of length l, one compare
 * finds the length -- works unchanged on 16 lanes: the ballot's 16 bits of the group, ds_bpermute inside the
 * group.  Headers and prefix-code tables are rare (a few per record) and use all 64 lanes through the shared
 * wave-cooperative code (brotli_dec_common.h), one group at a time.
 *
 * A wave with four streams is bound by the LATENCY of its dependent chain, not by issue (first version, measured:
 * one pass of the command loop ~6 400 cycles, most of them LDS round trips -- 26.2 GB/s), so the chain carries as few
 * LDS round trips as possible:
 *   - the bit buffer of a group is a 64-bit register pair; the next dword of the stream is read from the group's
 *     256-byte LDS window a whole refill ahead of its use, so no LDS access sits between two symbols;
 *   - every tree has a 256-entry direct table (payload | code length + 1 << 12) built with the tree: a symbol whose
 *     code has at most 8 bits costs ONE LDS read; longer codes (rare) take the canonical path -- the ballot's 16 bits
 *     of the group, two ds_bpermute, the sorted-symbol array;
 *   - up to 16 copies wait in a group's 16 lanes and are executed side by side with watermark rounds, as in
 *     brotli_dec.hip; literals are stored straight to their final positions.
 */
#include "brotli_dec_common.h"
#include "brotli_dec_rec.h"

#define B4_HANDOFF 102u /* internal status: zmt_brotli_dec_kernel decodes the record afterwards (gpumt.hip) */
#define B4_WIN 256u
#define B4_WSTRIDE (B4_WIN + 16u)
#ifndef B4_NB
#define B4_NB 16u /* copies a group holds back before it executes them (one per lane) */
#endif
#ifndef B4_NG
#define B4_NG 4u /* streams per wave (16-lane groups in use); gpumt.hip sizes the grid with the same number */
#endif

enum { B4_S_HDR = 0, B4_S_DEC = 1, B4_S_FIN = 2, B4_S_DONE = 3 };
#define B4_DIST_MAX 128u /* distance alphabet this kernel takes (NPOSTFIX = NDIRECT = 0 make 64); larger ones are handed over */
#define B4_DIST_STRIDE (128u + 2u * B4_DIST_MAX)
#define B4_T_LIT 0u
#define B4_T_CMD 1u
#define B4_T_DIST 2u

struct B4Lds {
	/* scratch of the shared prefix-code reader (br_read_code: one group at a time) */
	__attribute__((aligned(8))) u8 clrec[128 + 32];
	u8 lens[704];
	u8 tmp[64];
	u32 kins[24], kcopy[24]; /* insert / copy length codes: base | extra bits << 24 */
	/* per group: tree records (16 x u64 vector + sorted symbols), direct tables, stream window */
	__attribute__((aligned(8))) u8 lit[B4_NG][BR_LIT_STRIDE];
	__attribute__((aligned(8))) u8 cmd[B4_NG][BR_CMD_STRIDE];
	__attribute__((aligned(8))) u8 dist[B4_NG][B4_DIST_STRIDE];
	u16 tab[B4_NG][3][256]; /* payload | (code length + 1) << 12; 0 = the code is longer than 8 bits */
	__attribute__((aligned(16))) u8 win[B4_NG][B4_WSTRIDE];
};

/* direct table of a tree record: entry e = the symbol whose code opens the 8 stream bits e (first bit = bit 0), if
 * that code has at most 8 bits.  With the unknown bits behind the 8 taken as zeros the canonical compare finds the
 * same length as with the real ones whenever that length is <= 8 (the bounds of such lengths are multiples of 2^7) */
static __device__ __forceinline__ void b4_build_tab(const u8 *rec, u16 *tab, bool sym16, int lane)
{
	for (u32 e = (u32)lane; e < 256u; e += 64u) {
		const u32 c = br_rev15(e);
		u32 l = 9;
		for (int k = 8; k >= 0; k--)
			if (c < (*(const u32 *)(rec + 8 * k) & 0xFFFFu))
				l = (u32)k;
		u32 ent = 0;
		if (l <= 8u) {
			const u32 a = *(const u32 *)(rec + 8 * l), i0 = *(const u32 *)(rec + 8 * l + 4);
			const u32 idx = i0 + ((c - (a >> 16)) >> (15 - l));
			const u32 sym = sym16 ? (u32) * (const u16 *)(rec + 128 + 2 * idx) : (u32)rec[128 + idx];
			ent = (sym & 0xFFFu) | (l + 1u) << 12;
		}
		tab[e] = (u16)ent;
	}
}

/* order a group's earlier global stores before its later global loads, inside group-divergent control flow (the hardware
 * fence is the wave's; the fiber harness must not wait for lanes of other groups) */
static __device__ __forceinline__ void b4_grp_fence()
{
#ifdef ZMT_EMU
	grp_sync();
#else
	wave_mem_fence();
#endif
}

/* index of the next symbol in the sorted array of the tree whose vector this group's lanes hold (lane l of the group:
 * va / vi of code length l); *len = its code length */
static __device__ __forceinline__ u32 b4_sym_index(u32 bits, u32 va, u32 vi, u32 *len, bool &bad)
{
	const u32 c = br_rev15(bits & 0x7FFFu);
	const u32 m = grp_ballot(c < (va & 0xFFFFu));
	if (!m)
		bad = true;
	const int l = m ? wv_ffs((u64)m) - 1 : 0;
	const u32 a = grp_shfl(va, l), i0 = grp_shfl(vi, l);
	*len = (u32)l;
	return i0 + ((c - (a >> 16)) >> (15 - l));
}

/* copy of `ml` bytes at distance `off` by the 16 lanes of a group (long copies; plain or overlapping) */
static __device__ __forceinline__ void b4_grp_match(u8 *d, u32 off, u32 ml, u32 l16)
{
	const u8 *s = d - off;
	if (off >= ml) {
		const u32 body = ml & ~7u;
		for (u32 i = 8u * l16; i < body; i += 128u)
			st64g(d + i, ld64u(s + i));
		for (u32 i = body + l16; i < ml; i += 16u)
			d[i] = s[i];
	} else if (off >= 16u) {
		for (u32 done = 0; done < ml; done += off) {
			const u32 n = ml - done < off ? ml - done : off;
			for (u32 i = l16; i < n; i += 16u)
				d[done + i] = s[done + i];
			b4_grp_fence();
		}
	} else {
		for (u32 i = l16; i < ml; i += 16u)
			d[i] = s[i % off];
	}
}

/* What a 16-lane group decodes.  B4_RECORDS: record `u` of the batch.  B4_WANTED: the same, but only the records whose status
 * word is `want` on entry (the record pass of gpumt_brotli_decompress_batch_par: the others were decoded span by span).
 * B4_SPANS: entry `u` of a table of spans (B4Span, brotli_dec_rec.h) -- a byte range of a record that the record's index says
 * decodes on its own; whatever shows that it does not is a refusal (any status but ST_OK), never a verdict */
#define B4_RECORDS 0
#define B4_WANTED 1
#define B4_SPANS 2

#ifdef B4_WPE
#define B4_OCC __attribute__((amdgpu_waves_per_eu(B4_WPE, B4_WPE)))
#else
#define B4_OCC
#endif
#define B4_MODE B4_RECORDS
#define B4_NAME zmt_brotli_dec4_kernel
#include "brotli_dec4_body.h"
/* the record pass of gpumt_brotli_decompress_batch_par: the records whose status word is `want`, the others are passed by */
#define B4_MODE B4_WANTED
#define B4_NAME zmt_brotli_dec4_wanted_kernel
#include "brotli_dec4_body.h"
/* its execute stage: four spans per wave, status[u] = ST_OK where span u decoded to its stated length on its own */
#define B4_MODE B4_SPANS
#define B4_NAME zmt_brotli_dec4_span_kernel
#include "brotli_dec4_body.h"

#ifdef ZMT_EMU
/*
 * TEST HARNESS ONLY (tests/emu compiles this file as host C++): gpumt_brotli_decompress_batch_par over the fiber emulator, with
 * the shapes of include/gpumt.h, so that the span stages and the host engine's GPUMT_BROTLI_REC_PAR path run on the CPU.
 * Synchronous, host pointers stand in for device pointers.  Never part of the product.
 */
#include <vector>
#include "../../../include/gpumt.h"
extern "C" {
void zmt_brotli_dec_kernel(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *, const u32 *, u32 *, u32 *, u8 *, const u8 *,
			   u32);
void emu_brotli_decompress_batch(const u8 *stream, const u64 *rec_off, const u32 *rec_len, u32 nrec, u8 *out, const u64 *out_off,
				 const u32 *out_cap, u32 *out_len, u32 *status, const u8 *blob, u32 grid);
/* (the host engines' library has it; the kernels-only library, where only the emu_ entry is called, does not) */
extern const unsigned char zmt_brotli_static[] __attribute__((weak));

/* min_spans: "brotli_rec_min_spans"; cap: the scratch the "device" grants, 0 = any -- a request above it is refused and the
 * whole batch goes to the serial call; slice_spans: BREC_SLICE_SPANS, smaller for the tests.  info = eligible records, their
 * spans, records kept, fallback.  EMU_BROTLI_DEC=1 (the general kernel alone) as in emu_brotli_decompress_batch */
void emu_brotli_decompress_batch_par(const u8 *stream, const u64 *rec_off, const u32 *rec_len, u32 nrec, u8 *out,
				     const u64 *out_off, const u32 *out_cap, u32 *out_len, u32 *status, u32 *rec_par, const u8 *blob,
				     u32 grid, u32 min_spans, u64 cap, u32 slice_spans, u64 info[4])
{
	info[0] = info[1] = info[2] = info[3] = 0;
	if (rec_par)
		for (u32 i = 0; i < nrec; i++)
			rec_par[i] = 0;
	std::vector<BRec> recs(nrec);
	std::vector<u32> ufirst(nrec, 0xA5A5A5A5u);
	BRec *rp = recs.data();
	u32 *uf = ufirst.data();
	const u64 need_a = (u64)nrec * (sizeof(BRec) + 4);
	bool par = !(cap && need_a > cap);
	u32 max_span = 0, nslices = 0;
	BRecSlice S;
	if (par) {
		emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
			    [=]() { zmt_brotli_rec_plan_kernel(stream, rec_off, rec_len, nrec, out_off, out_cap, min_spans, rp); });
		for (size_t at = 0; brec_next_slice(rp, nrec, at, slice_spans, &S); at = S.b) {
			info[1] += S.nspan;
			nslices++;
			max_span = S.nspan > max_span ? S.nspan : max_span;
		}
		for (u32 i = 0; i < nrec; i++)
			info[0] += rp[i].flags & BREC_ELIGIBLE;
		if (cap && need_a + (u64)max_span * (sizeof(B4Span) + 4) > cap)
			par = false;
	}
	if (!par || !nslices) {
		info[0] = info[1] = 0;
		info[3] = par ? 0 : 1;
		emu_brotli_decompress_batch(stream, rec_off, rec_len, nrec, out, out_off, out_cap, out_len, status, blob, grid);
		return;
	}
	std::vector<B4Span> spans(max_span);
	std::vector<u32> span_st(max_span, 0xA5A5A5A5u);
	B4Span *sp = spans.data();
	u32 *ss = span_st.data();
	for (u32 i = 0; i < nrec; i++)
		status[i] = BREC_TODO;
	for (size_t at = 0; brec_next_slice(rp, nrec, at, slice_spans, &S); at = S.b) {
		const u32 n = (u32)(S.b - S.a), a = (u32)S.a, ns = S.nspan;
		emu::launch(emu::dim3{1, 1, 1}, emu::dim3{256, 1, 1}, [=]() { zmt_brotli_rec_scan_kernel(rp + a, n, uf + a); });
		emu::launch(emu::dim3{(n + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
			    [=]() { zmt_brotli_rec_table_kernel(stream, rp + a, n, a, uf + a, ns, sp); });
		emu::launch(emu::dim3{(ns + B4_NG - 1) / B4_NG, 1, 1}, emu::dim3{64, 1, 1},
			    [=]() { zmt_brotli_dec4_span_kernel(stream, sp, ns, out, ss); });
		emu::launch(emu::dim3{(n + 255) / 256, 1, 1}, emu::dim3{256, 1, 1}, [=]() {
			zmt_brotli_rec_finish_kernel(rp + a, n, uf + a, ns, sp, ss, out_len + a, status + a, rec_par ? rec_par + a : nullptr);
		});
	}
	for (u32 i = 0; i < nrec; i++)
		info[2] += status[i] == ST_OK;
	/* the record decoders over the records still marked */
	if (grid > nrec)
		grid = nrec;
	std::vector<u8> scr((size_t)grid * BR_WSCRATCH, 0xA5);
	u8 *sc = scr.data();
	const char *v = getenv("EMU_BROTLI_DEC");
	u32 want = BREC_TODO;
	if (!(v && atoi(v) == 1)) {
		emu::launch(emu::dim3{(nrec + B4_NG - 1) / B4_NG, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
			zmt_brotli_dec4_wanted_kernel(stream, rec_off, rec_len, nrec, out, out_off, out_cap, out_len, status, BREC_TODO);
		});
		want = B4_HANDOFF;
	}
	emu::launch(emu::dim3{grid, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_brotli_dec_kernel(stream, rec_off, rec_len, nrec, out, out_off, out_cap, out_len, status, sc, blob, want);
	});
}

/* (the emulated boundary keeps no variants: GPUMT_BROTLI_REC_MIN_SPANS and GPUMT_BROTLI_REC_CAP -- bytes -- stand in for
 * gpumt_set_variant's "brotli_rec_min_spans" and "brotli_rec_cap_mb") */
int gpumt_brotli_decompress_batch_par(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off, const uint32_t *d_rec_len,
				      size_t nrec, void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
				      uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int s)
{
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	const char *m = getenv("GPUMT_BROTLI_REC_MIN_SPANS"), *c = getenv("GPUMT_BROTLI_REC_CAP"), *t = getenv("GPUMT_TRACE");
	long mv = m && *m ? atol(m) : 2;
	if (mv < 2 || mv > 65536)
		mv = 2;
	u64 info[4];
	emu_brotli_decompress_batch_par((const u8 *)d_stream, d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off, d_out_cap,
					d_out_len, d_status, d_rec_par, zmt_brotli_static, 3, (u32)mv, c && *c ? strtoull(c, 0, 10) : 0,
					BREC_SLICE_SPANS, info);
	if (t && atoi(t) >= 1)
		fprintf(stderr, "[gpumt brotli rec] records %zu par %zu spans %zu kept %zu fallback %d\n", nrec, (size_t)info[0],
			(size_t)info[1], (size_t)info[2], (int)info[3]);
	return GPUMT_OK;
}
}
#endif
