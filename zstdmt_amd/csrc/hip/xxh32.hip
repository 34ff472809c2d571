/*
 * xxh32.hip -- batched XXH32 (seed 0) over many independent items (chunk contents).
 *
 * Replaces the XXH32 that LZ4F_compressFrame / LZ4F_decompress run over every chunk for the
 * content checksum (reference call sites lib/lz4-mt_compress.c:281, lib/lz4-mt_decompress.c:350;
 * flag set at lib/lz4-mt_compress.c:145).
 *
 * XXH32 is four independent serial accumulator chains per item (rotl/mul, not associative), so
 * the parallelism is across items: a quad of lanes owns one item, lane a of the quad runs
 * accumulator a.  A wave therefore streams 16 items; every wave-level load fetches 16 B from each
 * of them (the four lanes of a quad read one 16-byte stripe).
 * HBM-bound: algorithmic bytes = item length, read once.
 */
#include "lz4_common.h"

#ifndef XXH_BLOCK
#define XXH_BLOCK 256
#endif

extern "C" __global__ void __launch_bounds__(XXH_BLOCK)
zmt_xxh32_kernel(const u8 *__restrict__ base, const u64 *__restrict__ off,
		 const u32 *__restrict__ len, u32 n, u32 *__restrict__ out,
		 const u32 *__restrict__ expect, const u32 *__restrict__ expect_valid,
		 u32 *__restrict__ status)
{
	const u32 gtid = blockIdx.x * XXH_BLOCK + threadIdx.x;
	const u32 item = gtid >> 2;
	const u32 a = gtid & 3;
	const bool live = item < n;
	const u8 *p = live ? base + off[item] : base;
	const u32 L = live ? len[item] : 0;
	u32 v = 0;

	if (L >= 16) {
		u32 acc = (a == 0) ? XP1 + XP2 : (a == 1) ? XP2 : (a == 2) ? 0u : 0u - XP1;
		const u8 *q = p + a * 4;
		u32 ns = L >> 4, s = 0;
		for (; s + 4 <= ns; s += 4) {
			u32 x0 = ld32u(q), x1 = ld32u(q + 16), x2 = ld32u(q + 32), x3 = ld32u(q + 48);
			acc = xxh_round(acc, x0);
			acc = xxh_round(acc, x1);
			acc = xxh_round(acc, x2);
			acc = xxh_round(acc, x3);
			q += 64;
		}
		for (; s < ns; s++) {
			acc = xxh_round(acc, ld32u(q));
			q += 16;
		}
		v = rotl32(acc, (a == 0) ? 1 : (a == 1) ? 7 : (a == 2) ? 12 : 18);
	}
	/* quad reduction, wave-uniform */
	{
		int l = wv_lane();
		v += wv_shfl(v, l ^ 1);
		v += wv_shfl(v, l ^ 2);
	}
	if (live && a == 0) {
		u32 h = (L >= 16 ? v : XP5) + L;
		h = xxh_tail(h, p + (L & ~15u), L & 15);
		if (out)
			out[item] = h;
		if (expect && expect_valid[item] && expect[item] != h && status[item] == ST_OK)
			status[item] = ST_BAD_CHECKSUM;
	}
}

/*
 * XXH32 with carried state (gpumt_xxh32_carry): the content checksum of a plain .lz4 frame that is decoded batch after
 * batch.  The hash of a frame is one serial chain per accumulator and cannot be split, so a job continues a state over
 * the next piece of the frame's content and finalises it at the frame's end: one wave per job, lanes 0..3 run the four
 * accumulators over the 16-byte stripes, lane 0 keeps the up to 15 bytes that do not fill a stripe.  A state is 12
 * words in device memory: acc[4], pending count, total length lo / hi, spare, 16 pending bytes.  Jobs of one launch
 * run side by side, so the one that reads a carried state and the one that leaves one name different slots.
 */
struct XxhJob { /* == gpumt_xxh32_job */
	u64 off;
	u32 len, flags, expect, reserved;
};
#define XJ_RESET 1u   /* start a new hash instead of reading a state */
#define XJ_FINAL 2u   /* finalise: digest[j], and verdict[j] if XJ_VERIFY */
#define XJ_VERIFY 4u
#define XJ_IN(f) (((f) >> 8) & 1u)  /* state slot read */
#define XJ_OUT(f) (((f) >> 9) & 1u) /* state slot written */

extern "C" __global__ void __launch_bounds__(64)
zmt_xxh32_carry_kernel(const u8 *__restrict__ base, u64 base_bytes, const XxhJob *__restrict__ jobs, u32 njobs,
		       u32 *__restrict__ states, u32 *__restrict__ digest, u32 *__restrict__ verdict)
{
	const u32 j = blockIdx.x;
	const int lane = wv_lane();
	if (j >= njobs)
		return;
	const XxhJob J = jobs[j];
	if (J.off > base_bytes || J.len > base_bytes - J.off) {
		if (lane == 0) {
			digest[j] = 0;
			verdict[j] = ST_BAD_RECORD;
		}
		return;
	}
	const u32 a = (u32)lane & 3;
	const u32 *sin = states + 12 * XJ_IN(J.flags);
	u32 *sout = states + 12 * XJ_OUT(J.flags);
	u32 acc = (a == 0) ? XP1 + XP2 : (a == 1) ? XP2 : (a == 2) ? 0u : 0u - XP1;
	u32 npend = 0, pw = 0; /* pw: lane a's word of the pending stripe */
	u64 total = 0;
	if (!(J.flags & XJ_RESET)) {
		acc = sin[a];
		npend = sin[4] & 15u;
		total = (u64)sin[5] | (u64)sin[6] << 32;
		pw = sin[8 + a];
	}
	const u8 *p = base + J.off;
	u32 len = J.len;
	total += len;
	/* complete the pending stripe first: byte k of it is byte k - npend of the piece */
	if (npend) {
		const u32 take = 16 - npend < len ? 16 - npend : len;
		for (u32 k = 0; k < 4; k++) {
			const u32 at = 4 * a + k;
			if (at >= npend && at < npend + take)
				pw = (pw & ~(0xFFu << (8 * k))) | (u32)p[at - npend] << (8 * k);
		}
		p += take;
		len -= take;
		npend += take;
		if (npend == 16) {
			acc = xxh_round(acc, pw);
			npend = 0;
		}
	}
	if (lane < 4) {
		const u8 *q = p + a * 4;
		u32 ns = len >> 4, s = 0;
		for (; s + 8 <= ns; s += 8) {
			u32 x[8];
			for (u32 k = 0; k < 8; k++)
				x[k] = ld32u(q + 16 * k);
			for (u32 k = 0; k < 8; k++)
				acc = xxh_round(acc, x[k]);
			q += 128;
		}
		for (; s < ns; s++) {
			acc = xxh_round(acc, ld32u(q));
			q += 16;
		}
	}
	if (npend == 0) { /* (else the piece ended inside the pending stripe: len is 0) */
		const u8 *t = p + (len & ~15u);
		npend = len & 15;
		pw = 0;
		for (u32 k = 0; k < 4; k++)
			if (4 * a + k < npend)
				pw |= (u32)t[4 * a + k] << (8 * k);
	}
	if (J.flags & XJ_FINAL) {
		u32 v = lane < 4 ? rotl32(acc, (a == 0) ? 1 : (a == 1) ? 7 : (a == 2) ? 12 : 18) : 0;
		v += wv_shfl(v, lane ^ 1);
		v += wv_shfl(v, lane ^ 2);
		u32 h = (total >= 16 ? v : XP5) + (u32)total;
		u8 tail[16];
		for (u32 k = 0; k < 4; k++) {
			const u32 w = wv_readlane(pw, (int)k);
			tail[4 * k] = (u8)w;
			tail[4 * k + 1] = (u8)(w >> 8);
			tail[4 * k + 2] = (u8)(w >> 16);
			tail[4 * k + 3] = (u8)(w >> 24);
		}
		h = xxh_tail(h, tail, npend);
		if (lane == 0) {
			digest[j] = h;
			verdict[j] = (J.flags & XJ_VERIFY) && h != J.expect ? ST_BAD_CHECKSUM : ST_OK;
		}
	} else {
		if (lane < 4) {
			sout[a] = acc;
			sout[8 + a] = pw;
		}
		if (lane == 0) {
			sout[4] = npend;
			sout[5] = (u32)total;
			sout[6] = (u32)(total >> 32);
			sout[7] = 0;
			digest[j] = 0;
			verdict[j] = ST_OK;
		}
	}
}

#ifdef ZMT_EMU
/* TEST HARNESS ONLY (tests/emu compiles this file as host C++): gpumt_xxh32_carry over the fiber emulator, as the
 * block-level calls at the end of lz4_dec.hip.  Never part of the product. */
#include "../../../include/gpumt.h"
extern "C" {
void emu_xxh32_carry(const u8 *base, u64 base_bytes, const void *jobs, u32 njobs, u32 *states, u32 *digest, u32 *verdict)
{
	emu::launch(emu::dim3{njobs, 1, 1}, emu::dim3{64, 1, 1},
		    [=]() { zmt_xxh32_carry_kernel(base, base_bytes, (const XxhJob *)jobs, njobs, states, digest, verdict); });
}

int gpumt_xxh32_carry(gpumt_ctx *h, const void *d_base, size_t base_bytes, const gpumt_xxh32_job *d_jobs, size_t njobs,
		      uint32_t *d_states, uint32_t *d_digest, uint32_t *d_verdict, int s)
{
	static_assert(sizeof(gpumt_xxh32_job) == sizeof(XxhJob), "table layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_base || !d_jobs || !d_states || !d_digest || !d_verdict ||
	    njobs > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (njobs)
		emu_xxh32_carry((const u8 *)d_base, base_bytes, d_jobs, (u32)njobs, d_states, d_digest, d_verdict);
	return GPUMT_OK;
}
}
#endif
