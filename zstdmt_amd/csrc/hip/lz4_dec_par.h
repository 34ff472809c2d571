/*
 * lz4_dec_par.h -- the blocks of a linked run decoded side by side (gpumt_lz4_decompress_blocks_par); included by
 * lz4_dec.hip behind the serial run decoder, whose results these launches reproduce.
 *
 * A block of a linked frame may copy from the up to 64 KiB of output in front of it, i.e. from bytes another block
 * produces.  What a block's own bytes are is known without them, except for the bytes that come from before its start:
 * so every block is decoded at its final position by a wave of its own, a match source below the block's first byte is
 * not read but written down (an "origin": how far before the block's start the byte comes from), and a last launch
 * fills those bytes in, block after block.  No wave waits for another wave of its launch; the order comes from the
 * launches being stream-ordered and from a workgroup's barrier.
 *
 *   plan     one wave: the runs of two or more blocks must lie in ascending, disjoint block ranges (the host engine's
 *            tables do); then owner[b] = the run of block b.  Any other table decodes with the serial code, all of it.
 *   measure  one wave per block of such a run: table entry, block checksum, and a token walk without copying ->
 *            decoded length and everything of the verdict that does not depend on the history.
 *   scan     one wave per run: positions from the lengths, the room checks, the first block that fails; every other run
 *            (one block, or a refused table entry) is decoded here by lz4_run_serial.
 *   execute  one wave per block in front of its run's first failing block.  The run's first block has its history in
 *            memory and is decode_block_serial; a later block writes values and, per output byte, a u16 origin: 0 =
 *            the value is there, d = the value is the byte d before the block's first.  A match inside the block copies
 *            value and origin alike, so a byte copied three times still names where it came from.
 *   resolve  one workgroup per run, blocks in order: out[p] = out[block start - origin[p]] wherever origin[p] != 0.
 *            Everything before the block is final by then.  Then block lengths, run length and status, those of the
 *            first failing block in block order.
 */
#ifndef ZMT_LZ4_DEC_PAR_H
#define ZMT_LZ4_DEC_PAR_H

#define LZ4P_NONE 0xFFFFFFFFu
#define LZ4P_UNRES 0x100u /* xst: the block left origins behind */

/* scratch of one call; the five block arrays and `origin` (one entry per byte of d_out) are device memory */
struct Lz4Par {
	u16 *origin;
	u32 *owner; /* run of the block, LZ4P_NONE: of no run of two or more blocks (memset by the host) */
	u32 *mlen;  /* measured length */
	u32 *mst;   /* verdict of measure, then of scan's room check */
	u32 *pos;   /* position in the run's area, from R.low; LZ4P_NONE: not executed */
	u32 *xst;   /* verdict of execute | LZ4P_UNRES */
	u32 *flag;  /* [0] = the plan holds */
};

static __device__ __forceinline__ void wave_zero16(u16 *d, u32 n, int lane)
{
	u32 i = 0;
	if (n >= 256) {
		const u32 n2 = n & ~127u;
		for (i = (u32)lane * 2; i < n2; i += 128)
			st32u((u8 *)(d + i), 0);
		i = n2;
	}
	for (i += (u32)lane; i < n; i += 64)
		d[i] = 0;
}

/*
 * decode_block_serial's walk over one block whose history is not in memory.
 * EXEC = 0 (measure): nothing is copied, opos counts from 0 and limit is the block maximum; history is not judged.
 * EXEC = 1: the block starts at out[opos] = the run's area from R.low; values and origins are written, a match source
 * below the block's start is written down instead of read; `off > opos` is the serial decoder's history check (low = 0).
 * Returns the new opos or LZ4P_NONE.
 */
template <int EXEC>
static __device__ u32 decode_block_par(const u8 *src, u32 slen, u8 *out, u16 *org, u32 opos, u32 limit, u32 blkmax,
				       int lane, bool &unres)
{
	u32 ip = 0;
	const u32 opos0 = opos;
	bool un = false;
	if (slen == 0)
		return LZ4P_NONE;
	for (;;) {
		u32 tok, lit, ml, off, t;
		if (ip >= slen)
			return LZ4P_NONE;
		t = ip;
		tok = uld8(src + ip++);
		lit = tok >> 4;
		if (lit == 15) {
			u32 b;
			if (slen - ip <= 15)
				return LZ4P_NONE;
			do {
				if (ip >= slen)
					return LZ4P_NONE;
				b = uld8(src + ip++);
				lit += b;
			} while (b == 255);
		}
		if (slen - ip < lit || limit - opos < lit)
			return LZ4P_NONE;
		if (slen - ip > lit && lz4lib_tail_bad(t, ip, lit, opos - opos0, slen, blkmax))
			return LZ4P_NONE;
		if (EXEC) {
			wave_copy(out + opos, src + ip, lit, lane);
			wave_zero16(org + opos, lit, lane);
		}
		ip += lit;
		opos += lit;
		if (ip == slen) {
			unres = wv_any(un);
			return opos;
		}
		if (slen - ip < 2)
			return LZ4P_NONE;
		off = uld16(src + ip);
		ip += 2;
		ml = tok & 15;
		if (ml == 15) {
			u32 b;
			do {
				if (ip >= slen)
					return LZ4P_NONE;
				b = uld8(src + ip++);
				ml += b;
			} while (b == 255);
			if (slen - ip < 5)
				return LZ4P_NONE;
		}
		ml += 4;
		if (off == 0 || (EXEC && off > opos) || limit - opos < ml)
			return LZ4P_NONE;
		if (lz4lib_match_tail_bad(t, tok, off, opos - opos0 - lit, lit + ml, slen, blkmax))
			return LZ4P_NONE;
		if (EXEC) {
			const u32 mp = opos - off;
			wave_mem_fence();
			if (mp >= opos0) { /* the whole source is the block's own */
				if (off >= ml) {
					for (u32 i = (u32)lane; i < ml; i += 64) {
						const u32 o = org[mp + i];
						out[opos + i] = out[mp + i];
						org[opos + i] = (u16)o;
					}
				} else {
					for (u32 i = (u32)lane; i < ml; i += 64) {
						const u32 si = mp + i % off;
						out[opos + i] = out[si];
						org[opos + i] = org[si];
					}
				}
			} else { /* it starts before the block: bytewise; with off < ml byte i is byte i mod off of the source */
				for (u32 i = (u32)lane; i < ml; i += 64) {
					const u32 si = mp + (off >= ml ? i : i % off);
					if (si < opos0) {
						org[opos + i] = (u16)(opos0 - si); /* 1 .. off */
						un = true;
					} else {
						out[opos + i] = out[si];
						org[opos + i] = org[si];
					}
				}
			}
		}
		opos += ml;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_par_plan_kernel(const Lz4Run *__restrict__ runs, u32 nrun, u32 nblk, u64 out_bytes, Lz4Par P)
{
	const int lane = wv_lane();
	u32 hi = 0; /* end of the block ranges so far */
	bool bad = false;
	if (blockIdx.x != 0)
		return;
	for (int pass = 0; pass < 2; pass++) {
		const bool ordered = pass ? !wv_any(bad) : false;
		if (pass && !ordered)
			break;
		for (u32 base = 0; base < nrun; base += 64) {
			const u32 r = base + (u32)lane;
			u32 first = 0, count = 0;
			if (r < nrun) {
				const Lz4Run R = runs[r];
				if (lz4_run_ok(R, nblk, out_bytes) && R.count >= 2) {
					first = R.first;
					count = R.count;
				}
			}
			if (!pass) {
				const u32 inc = wv_scan_max_incl(count ? first + count : 0);
				u32 before = wv_shr1(inc, 0);
				if (before < hi)
					before = hi;
				if (count && first < before)
					bad = true;
				const u32 top = wv_shfl(inc, 63);
				if (top > hi)
					hi = top;
			} else {
				for (u64 m = wv_ballot(count != 0); m; m &= m - 1) {
					const int l = wv_ffs(m) - 1;
					const u32 f = wv_shfl(first, l), c = wv_shfl(count, l);
					for (u32 i = (u32)lane; i < c; i += 64)
						P.owner[f + i] = base + (u32)l;
				}
			}
		}
		if (pass && lane == 0)
			P.flag[0] = 1;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_par_measure_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const Lz4Block *__restrict__ blocks, u32 nblk,
			   Lz4Par P)
{
	const u32 b = blockIdx.x;
	const int lane = wv_lane();
	if (b >= nblk || !wv_readfirst(P.flag[0]) || wv_readfirst(P.owner[b]) == LZ4P_NONE)
		return;
	const Lz4Block B = blocks[b];
	const u32 bsz = wv_readfirst(B.src_len), bm = wv_readfirst(B.blkmax);
	const u8 *src = stream + B.src_off;
	u32 st = ST_OK, len = 0;
	if (B.src_off > stream_bytes || bsz > stream_bytes - B.src_off || bm < 65536u || bm > (4u << 20)) {
		st = ST_BAD_RECORD;
	} else if (bsz > bm) {
		st = ST_BAD_BLOCK;
	} else if ((B.flags & LZ4B_CHECKSUM) && wave_xxh32(src, bsz, lane) != wv_readfirst(B.checksum)) {
		st = ST_BAD_CHECKSUM;
	} else if (B.flags & LZ4B_STORED) {
		len = bsz;
	} else {
		bool un;
		len = decode_block_par<0>(src, bsz, NULL, NULL, 0, bm, bm, lane, un);
		if (len == LZ4P_NONE)
			st = ST_BAD_BLOCK;
	}
	if (lane == 0) {
		P.mst[b] = st;
		P.mlen[b] = len;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_par_scan_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const Lz4Block *__restrict__ blocks, u32 nblk,
			const Lz4Run *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes, u32 *__restrict__ blk_len,
			u32 *__restrict__ run_len, u32 *__restrict__ status, Lz4Par P)
{
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (r >= nrun)
		return;
	const Lz4Run R = runs[r];
	if (!wv_readfirst(P.flag[0]) || !lz4_run_ok(R, nblk, out_bytes) || R.count < 2) {
		lz4_run_serial(stream, stream_bytes, blocks, nblk, R, r, out_base, out_bytes, blk_len, run_len, status, lane);
		return;
	}
	const u64 end = (u64)(R.out_off - R.low) + R.out_cap;
	u64 at = R.out_off - R.low;
	bool failed = false;
	for (u32 base = 0; base < R.count; base += 64) {
		const u32 i = base + (u32)lane, b = R.first + i;
		const bool act = i < R.count;
		u32 st = ST_OK, len = 0;
		if (act) {
			st = P.mst[b];
			len = st == ST_OK ? P.mlen[b] : 0;
		}
		const u32 inc = wv_scan_incl(len); /* a length is at most 4 MiB */
		const u64 p = at + (inc - len);
		/* the serial decoder's room: a stored block must fit, a compressed one may not decode past the area's end */
		const bool bad = act && (st != ST_OK || p > end || end - p < len);
		const u64 m = wv_ballot(bad);
		const int fl = failed ? 0 : m ? wv_ffs(m) - 1 : 64; /* lanes below fl are executed */
		if (act) {
			P.pos[b] = lane < fl ? (u32)p : LZ4P_NONE;
			if (!failed && lane == fl && st == ST_OK)
				P.mst[b] = ST_BAD_BLOCK; /* the run's first failing block, for want of room */
		}
		if (m)
			failed = true;
		at += wv_shfl(inc, 63);
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_par_exec_kernel(const u8 *__restrict__ stream, const Lz4Block *__restrict__ blocks, u32 nblk,
			const Lz4Run *__restrict__ runs, u8 *out_base, Lz4Par P)
{
	const u32 b = blockIdx.x;
	const int lane = wv_lane();
	if (b >= nblk || !wv_readfirst(P.flag[0]))
		return;
	const u32 r = wv_readfirst(P.owner[b]);
	if (r == LZ4P_NONE)
		return;
	const u32 p = wv_readfirst(P.pos[b]);
	if (p == LZ4P_NONE)
		return;
	/* measure and scan have checked the entries: [p, p + mlen) lies inside the run's area */
	const Lz4Run R = runs[r];
	const Lz4Block B = blocks[b];
	const u32 bsz = wv_readfirst(B.src_len), bm = wv_readfirst(B.blkmax);
	const u32 end = wv_readfirst((u32)(R.out_off - R.low) + R.out_cap);
	const u8 *src = stream + B.src_off;
	u8 *out = out_base + R.low;
	u32 x = ST_OK;
	if (B.flags & LZ4B_STORED) {
		wave_copy(out + p, src, bsz, lane);
	} else {
		const u32 room = end - p < bm ? end - p : bm;
		bool un = false;
		u32 np;
		if (b == R.first)
			np = decode_block_serial(src, bsz, out, p, 0, p + room, bm, lane);
		else
			np = decode_block_par<1>(src, bsz, out, P.origin + R.low, p, p + room, bm, lane, un);
		x = np == LZ4P_NONE ? (u32)ST_BAD_BLOCK : un ? LZ4P_UNRES : (u32)ST_OK;
	}
	if (lane == 0)
		P.xst[b] = x;
}

#define LZ4P_RESOLVE_THREADS 1024
extern "C" __global__ void __launch_bounds__(LZ4P_RESOLVE_THREADS)
zmt_lz4_par_resolve_kernel(const Lz4Run *__restrict__ runs, u32 nrun, u32 nblk, u8 *out_base, u64 out_bytes,
			   u32 *__restrict__ blk_len, u32 *__restrict__ run_len, u32 *__restrict__ status, Lz4Par P)
{
	__shared__ u32 s_back; /* count - index of the first failing block */
	const u32 r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
	if (r >= nrun || !P.flag[0])
		return;
	const Lz4Run R = runs[r];
	if (!lz4_run_ok(R, nblk, out_bytes) || R.count < 2)
		return;
	if (tid == 0)
		s_back = 0;
	__syncthreads();
	for (u32 i = tid; i < R.count; i += nt)
		if (P.pos[R.first + i] == LZ4P_NONE || (P.xst[R.first + i] & 0xFFu) != ST_OK)
			atomicMax(&s_back, R.count - i);
	__syncthreads();
	const u32 nok = R.count - s_back;
	u8 *out = out_base + R.low;
	const u16 *org = P.origin + R.low;
	for (u32 i = 1; i < nok; i++) {
		const u32 b = R.first + i;
		if (!(P.xst[b] & LZ4P_UNRES))
			continue; /* (the same for every thread) */
		const u32 S = P.pos[b], L = P.mlen[b], L4 = L & ~3u;
		for (u32 j = tid * 4; j < L4; j += nt * 4) {
			const u64 o4 = ld64u((const u8 *)(org + S + j));
			if (!o4)
				continue;
			for (u32 k = 0; k < 4; k++) {
				const u32 o = (u32)(o4 >> (16 * k)) & 0xFFFFu;
				if (o)
					out[S + j + k] = out[S - o];
			}
		}
		if (tid < L - L4) {
			const u32 o = org[S + L4 + tid];
			if (o)
				out[S + L4 + tid] = out[S - o];
		}
		/* block i is final before block i + 1 reads it */
#ifndef ZMT_EMU
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#endif
		__syncthreads();
#ifndef ZMT_EMU
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
	}
	for (u32 i = tid; i < nok; i += nt)
		blk_len[R.first + i] = P.mlen[R.first + i];
	if (tid == 0) {
		const u32 start = (u32)(R.out_off - R.low);
		run_len[r] = nok ? P.pos[R.first + nok - 1] + P.mlen[R.first + nok - 1] - start : 0;
		status[r] = nok == R.count                         ? (u32)ST_OK
			    : P.pos[R.first + nok] == LZ4P_NONE ? P.mst[R.first + nok]
								: (u32)ST_BAD_BLOCK;
	}
}

#endif
