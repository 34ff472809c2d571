/*
 * lz4_dec_seg.h -- big plain .lz4 blocks decoded segment-parallel (gpumt_lz4_decompress_blocks_seg); included by
 * lz4_dec.hip behind lz4_dec_par.h, whose scheme this is with another unit.
 *
 * lz4_dec_par.h decodes the blocks of a linked run side by side: a byte that comes from before a block's first byte is
 * written down as an origin (its distance before the block's start, at most 65535 because an offset is 16 bits) and
 * filled in by a last, ordered launch.  Nothing there needs the unit to be a block: the origin of a byte lies at most
 * 65535 before any cut of the output.  What a wave needs to start in the middle of a block is a cut on a sequence
 * boundary -- the input position of a token and the output position it starts at -- and measure's token walk passes all
 * of them.  So the unit is a segment: the sequences of one block from the first token that starts at or behind
 * k * seg_bytes to the first one that starts at or behind (k + 1) * seg_bytes.  A 4 MiB block is 64 waves at the
 * default 64 KiB instead of one, whether it is independent (a run of its own) or one of a linked run.  A sequence
 * longer than a segment stays on one wave.  No wave waits for another wave of its launch.
 *
 *   plan     one wave: every run of one block or more must lie in ascending, disjoint block ranges; owner[b] = the run
 *            of block b.  Then the cuts block b can have at most: (min(blkmax, 255 x src_len or src_len when stored,
 *            out_cap) - 1) / seg_bytes, and cbase[] = their exclusive scan: block b's cuts live at cut[cbase[b]...], its
 *            segments are the slots cbase[b] + b ...  A run of one block that can have no cut is left to the serial code.
 *            A table that is not in order, or whose cuts do not fit the table (the runs' areas overlap), decodes with
 *            the serial code, all of it.
 *   measure  one wave per block: lz4_dec_par.h's measure, and a cut (ip, opos), block-relative, at the first token whose
 *            output position is >= k * seg_bytes, k = 1, 2, ...; a stored block is cut at k * seg_bytes.
 *   scan     one wave per run: positions, room, the first failing block.  Runs the plan left out, and a run of one block
 *            that turned out no longer than a segment, are decoded here by lz4_run_serial.
 *   execute  one wave per slot; the slot's block by bisection of cbase[].  The run's first segment has its history in
 *            memory; any other one does not read below its own first byte but writes origins, relative to the
 *            segment's start.  The end-of-block rules and the history check see block-relative ip / opos and the run's
 *            position as the serial decoder does: they come from the cut and from scan.
 *   resolve  one workgroup per run, segments in order, a barrier in between; then block lengths, run length, status and
 *            the number of segments of every block in front of the first failing one.
 */
#ifndef ZMT_LZ4_DEC_SEG_H
#define ZMT_LZ4_DEC_SEG_H

#define LZ4S_SERIAL 0xFFFFFFFEu /* pos: scan decoded the run's one block with the serial code */

/* scratch of one call, device memory */
struct Lz4Seg {
	u16 *origin;
	u32 *owner; /* [nblk] run of the block, LZ4P_NONE: the serial code's (memset by the host) */
	u32 *mlen;  /* [nblk] measured length */
	u32 *mst;   /* [nblk] verdict of measure, then of scan's room check */
	u32 *pos;   /* [nblk] position in the run's area, from R.low; LZ4P_NONE: not executed */
	u32 *nseg;  /* [nblk] measured segments */
	u32 *cbase; /* [nblk + 1] exclusive scan of the cuts a block can have */
	u32 *cut;   /* [2 * ncut] ip, opos of a cut, both block-relative */
	u32 *xst;   /* [ncut + nblk] per slot: verdict of execute | LZ4P_UNRES */
	u32 *flag;  /* [0] = the plan holds */
	u32 shift;  /* seg_bytes = 1 << shift */
	u32 ncut;   /* room of `cut` */
};

/*
 * decode_block_serial's walk over a part of one block.
 * MODE 0 (measure): nothing is copied, opos counts from 0, limit is the block maximum, history is not judged; the cuts
 *   go to cut[] (at most cutcap are written), ncut = how many there are.
 * MODE 1, 2 (execute): the tokens from ip to ipend (ipend = slen: to the block's end), the segment starting at out[opos]
 *   in the run's area from R.low, the block at out[opos0].  1: values and origins, a match source below the segment's
 *   start is written down instead of read.  2: the history is in memory (the run's first segment).
 * Returns the new opos or LZ4P_NONE.
 */
template <int MODE>
static __device__ u32 lz4s_walk(const u8 *src, u32 slen, u32 ip, u32 ipend, u8 *out, u16 *org, u32 opos0, u32 opos,
				u32 limit, u32 blkmax, int lane, bool &unres, u32 shift, u32 *cut, u32 cutcap, u32 &ncut)
{
	const u32 seg0 = opos;
	u32 next = 1u << shift, nc = 0, lastcut = LZ4P_NONE;
	bool un = false;
	if (slen == 0)
		return LZ4P_NONE;
	for (;;) {
		u32 tok, lit, ml, off, t;
		if (MODE != 0 && ipend < slen && ip >= ipend) { /* the next segment's first token */
			unres = wv_any(un);
			return opos;
		}
		if (ip >= slen)
			return LZ4P_NONE;
		if (MODE == 0 && opos >= next) {
			if (nc < cutcap && lane == 0) {
				cut[2 * nc] = ip;
				cut[2 * nc + 1] = opos;
			}
			nc++;
			lastcut = opos;
			next = ((opos >> shift) + 1) << shift;
		}
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
		if (MODE != 0)
			wave_copy(out + opos, src + ip, lit, lane);
		if (MODE == 1)
			wave_zero16(org + opos, lit, lane);
		ip += lit;
		opos += lit;
		if (ip == slen) {
			if (MODE == 0)
				ncut = lastcut == opos ? nc - 1 : nc; /* (a last token without literals starts no segment) */
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
		if (off == 0 || (MODE != 0 && off > opos) || limit - opos < ml)
			return LZ4P_NONE;
		if (lz4lib_match_tail_bad(t, tok, off, opos - opos0 - lit, lit + ml, slen, blkmax))
			return LZ4P_NONE;
		if (MODE == 2) {
			const u8 *m = out + opos - off;
			u8 *d = out + opos;
			wave_mem_fence();
			if (off >= ml) {
				for (u32 i = (u32)lane; i < ml; i += 64)
					d[i] = m[i];
			} else {
				for (u32 i = (u32)lane; i < ml; i += 64)
					d[i] = m[i % off];
			}
		}
		if (MODE == 1) {
			const u32 mp = opos - off;
			wave_mem_fence();
			if (mp >= seg0) { /* the whole source is the segment's own */
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
			} else { /* it starts before the segment: bytewise; with off < ml byte i is byte i mod off of the source */
				for (u32 i = (u32)lane; i < ml; i += 64) {
					const u32 si = mp + (off >= ml ? i : i % off);
					if (si < seg0) {
						org[opos + i] = (u16)(seg0 - si); /* 1 .. off */
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
zmt_lz4_seg_plan_kernel(const Lz4Block *__restrict__ blocks, u32 nblk, const Lz4Run *__restrict__ runs, u32 nrun,
			u64 out_bytes, Lz4Seg P)
{
	const int lane = wv_lane();
	u32 hi = 0; /* end of the block ranges so far */
	bool bad = false;
	if (blockIdx.x != 0)
		return;
	for (int pass = 0; pass < 2; pass++) {
		if (pass && wv_any(bad))
			return;
		for (u32 base = 0; base < nrun; base += 64) {
			const u32 r = base + (u32)lane;
			u32 first = 0, count = 0;
			if (r < nrun) {
				const Lz4Run R = runs[r];
				if (lz4_run_ok(R, nblk, out_bytes)) {
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
	}
	wave_mem_fence();
	u64 tot = 0;
	for (u32 base = 0; base < nblk; base += 64) {
		const u32 b = base + (u32)lane;
		u32 wc = 0;
		if (b < nblk) {
			const u32 r = P.owner[b];
			if (r != LZ4P_NONE) {
				const Lz4Block B = blocks[b];
				const u32 cap = runs[r].out_cap, one = runs[r].count == 1;
				u64 m = (B.flags & LZ4B_STORED) ? (u64)B.src_len : 255ull * B.src_len;
				if (m > (B.blkmax < (4u << 20) ? B.blkmax : (4u << 20)))
					m = B.blkmax < (4u << 20) ? B.blkmax : (4u << 20);
				if (m > cap)
					m = cap;
				wc = m ? (u32)((m - 1) >> P.shift) : 0;
				if (one && wc == 0)
					P.owner[b] = LZ4P_NONE; /* no longer than a segment whatever it holds */
			}
		}
		const u32 inc = wv_scan_incl(wc); /* a block has at most 4 MiB / 256 cuts */
		if (b < nblk)
			P.cbase[b] = (u32)tot + (inc - wc);
		tot += wv_shfl(inc, 63);
		if (tot > P.ncut)
			return;
	}
	if (lane == 0) {
		P.cbase[nblk] = (u32)tot;
		P.flag[0] = 1;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_seg_measure_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const Lz4Block *__restrict__ blocks, u32 nblk,
			   Lz4Seg P)
{
	const u32 b = blockIdx.x;
	const int lane = wv_lane();
	if (b >= nblk || !wv_readfirst(P.flag[0]) || wv_readfirst(P.owner[b]) == LZ4P_NONE)
		return;
	const Lz4Block B = blocks[b];
	const u32 bsz = wv_readfirst(B.src_len), bm = wv_readfirst(B.blkmax);
	const u32 c0 = wv_readfirst(P.cbase[b]), c1 = wv_readfirst(P.cbase[b + 1]);
	const u8 *src = stream + B.src_off;
	u32 st = ST_OK, len = 0, ns = 1;
	if (B.src_off > stream_bytes || bsz > stream_bytes - B.src_off || bm < 65536u || bm > (4u << 20)) {
		st = ST_BAD_RECORD;
	} else if (bsz > bm) {
		st = ST_BAD_BLOCK;
	} else if ((B.flags & LZ4B_CHECKSUM) && wave_xxh32(src, bsz, lane) != wv_readfirst(B.checksum)) {
		st = ST_BAD_CHECKSUM;
	} else if (B.flags & LZ4B_STORED) {
		len = bsz;
		ns = bsz ? ((bsz - 1) >> P.shift) + 1 : 1;
	} else {
		bool un;
		u32 nc = 0;
		len = lz4s_walk<0>(src, bsz, 0, bsz, NULL, NULL, 0, 0, bm, bm, lane, un, P.shift, P.cut + 2 * (size_t)c0, c1 - c0, nc);
		if (len == LZ4P_NONE)
			st = ST_BAD_BLOCK;
		else
			ns = nc + 1;
	}
	if (lane == 0) {
		P.mst[b] = st;
		P.mlen[b] = len;
		P.nseg[b] = ns;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_lz4_seg_scan_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const Lz4Block *__restrict__ blocks, u32 nblk,
			const Lz4Run *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes, u32 *__restrict__ blk_len,
			u32 *__restrict__ run_len, u32 *__restrict__ status, Lz4Seg P)
{
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (r >= nrun)
		return;
	const Lz4Run R = runs[r];
	bool serial = !wv_readfirst(P.flag[0]) || !lz4_run_ok(R, nblk, out_bytes) || R.count == 0 ||
		      wv_readfirst(P.owner[R.first]) == LZ4P_NONE;
	if (!serial && R.count == 1 && wv_readfirst(P.mst[R.first]) == ST_OK && wv_readfirst(P.nseg[R.first]) <= 1) {
		serial = true; /* one block of one segment: nothing to decode side by side */
		if (lane == 0)
			P.pos[R.first] = LZ4S_SERIAL;
	}
	if (serial) {
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
		bool fits = true;
		if (act) {
			st = P.mst[b];
			len = st == ST_OK ? P.mlen[b] : 0;
			fits = st != ST_OK || P.nseg[b] - 1 <= P.cbase[b + 1] - P.cbase[b];
		}
		const u32 inc = wv_scan_incl(len); /* a length is at most 4 MiB */
		const u64 p = at + (inc - len);
		/* the serial decoder's room: a stored block must fit, a compressed one may not decode past the area's end
		 * (a block with more cuts than the plan gave it room for is longer than out_cap: it fails this as well) */
		const bool bad = act && (st != ST_OK || p > end || end - p < len || !fits);
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
zmt_lz4_seg_exec_kernel(const u8 *__restrict__ stream, const Lz4Block *__restrict__ blocks, u32 nblk,
			const Lz4Run *__restrict__ runs, u8 *out_base, Lz4Seg P)
{
	const u32 s = blockIdx.x;
	const int lane = wv_lane();
	if (!nblk || !wv_readfirst(P.flag[0]) || s >= wv_readfirst(P.cbase[nblk]) + nblk)
		return;
	/* the block whose slots hold s: cbase[lo] + lo <= s < cbase[hi] + hi */
	u32 lo = 0, hi = nblk;
	while (hi - lo > 1) {
		const u32 mid = lo + (hi - lo) / 2;
		if (wv_readfirst(P.cbase[mid]) + mid <= s)
			lo = mid;
		else
			hi = mid;
	}
	const u32 b = lo, c0 = wv_readfirst(P.cbase[b]), k = s - (c0 + b);
	const u32 r = wv_readfirst(P.owner[b]);
	if (r == LZ4P_NONE)
		return;
	const u32 p = wv_readfirst(P.pos[b]);
	if (p == LZ4P_NONE || p == LZ4S_SERIAL)
		return;
	const u32 ns = wv_readfirst(P.nseg[b]);
	if (k >= ns)
		return;
	/* measure and scan have checked the entries: [p, p + mlen) lies inside the run's area, the cuts inside the table */
	const Lz4Run R = runs[r];
	const Lz4Block B = blocks[b];
	const u32 bsz = wv_readfirst(B.src_len), bm = wv_readfirst(B.blkmax);
	const u32 end = wv_readfirst((u32)(R.out_off - R.low) + R.out_cap);
	const u8 *src = stream + B.src_off;
	u8 *out = out_base + R.low;
	u32 x = ST_OK;
	if (B.flags & LZ4B_STORED) {
		const u32 a = k << P.shift, n = bsz - a < (1u << P.shift) ? bsz - a : (1u << P.shift);
		wave_copy(out + p + a, src + a, n, lane);
	} else {
		const u32 *cut = P.cut + 2 * (size_t)c0;
		const u32 ip0 = k ? wv_readfirst(cut[2 * (k - 1)]) : 0, op0 = k ? wv_readfirst(cut[2 * (k - 1) + 1]) : 0;
		const u32 ip1 = k + 1 < ns ? wv_readfirst(cut[2 * k]) : bsz;
		const u32 room = end - p < bm ? end - p : bm;
		bool un = false;
		u32 np, nc = 0;
		if (b == R.first && k == 0)
			np = lz4s_walk<2>(src, bsz, ip0, ip1, out, NULL, p, p + op0, p + room, bm, lane, un, P.shift, NULL, 0, nc);
		else
			np = lz4s_walk<1>(src, bsz, ip0, ip1, out, P.origin + R.low, p, p + op0, p + room, bm, lane, un, P.shift, NULL,
					  0, nc);
		x = np == LZ4P_NONE ? (u32)ST_BAD_BLOCK : un ? LZ4P_UNRES : (u32)ST_OK;
	}
	if (lane == 0)
		P.xst[s] = x;
}

extern "C" __global__ void __launch_bounds__(LZ4P_RESOLVE_THREADS)
zmt_lz4_seg_resolve_kernel(const Lz4Run *__restrict__ runs, u32 nrun, u32 nblk, u8 *out_base, u64 out_bytes,
			   u32 *__restrict__ blk_len, u32 *__restrict__ run_len, u32 *__restrict__ status,
			   u32 *__restrict__ blk_seg, Lz4Seg P)
{
	__shared__ u32 s_back; /* count - index of the first failing block */
	const u32 r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
	if (r >= nrun || !P.flag[0])
		return;
	const Lz4Run R = runs[r];
	if (!lz4_run_ok(R, nblk, out_bytes) || R.count == 0 || P.owner[R.first] == LZ4P_NONE || P.pos[R.first] == LZ4S_SERIAL)
		return;
	if (tid == 0)
		s_back = 0;
	__syncthreads();
	for (u32 i = tid; i < R.count; i += nt) {
		const u32 b = R.first + i, s0 = P.cbase[b] + b;
		bool bad = P.pos[b] == LZ4P_NONE;
		for (u32 k = 0; !bad && k < P.nseg[b]; k++)
			bad = (P.xst[s0 + k] & 0xFFu) != ST_OK;
		if (bad)
			atomicMax(&s_back, R.count - i);
	}
	__syncthreads();
	const u32 nok = R.count - s_back;
	u8 *out = out_base + R.low;
	const u16 *org = P.origin + R.low;
	for (u32 i = 0; i < nok; i++) {
		const u32 b = R.first + i, c0 = P.cbase[b], ns = P.nseg[b], S0 = P.pos[b];
		const u32 *cut = P.cut + 2 * (size_t)c0;
		for (u32 k = 0; k < ns; k++) {
			if (!(P.xst[c0 + b + k] & LZ4P_UNRES))
				continue; /* (the same for every thread) */
			const u32 S = S0 + (k ? cut[2 * (k - 1) + 1] : 0), E = S0 + (k + 1 < ns ? cut[2 * k + 1] : P.mlen[b]);
			const u32 L = E - S, L4 = L & ~3u;
			for (u32 j = tid * 4; j < L4; j += nt * 4) {
				const u64 o4 = ld64u((const u8 *)(org + S + j));
				if (!o4)
					continue;
				for (u32 q = 0; q < 4; q++) {
					const u32 o = (u32)(o4 >> (16 * q)) & 0xFFFFu;
					if (o && o <= S) /* (o <= S: execute's history check) */
						out[S + j + q] = out[S - o];
				}
			}
			if (tid < L - L4) {
				const u32 o = org[S + L4 + tid];
				if (o && o <= S)
					out[S + L4 + tid] = out[S - o];
			}
			/* this segment is final before the next one reads it */
#ifndef ZMT_EMU
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#endif
			__syncthreads();
#ifndef ZMT_EMU
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
		}
	}
	for (u32 i = tid; i < nok; i += nt) {
		blk_len[R.first + i] = P.mlen[R.first + i];
		blk_seg[R.first + i] = P.nseg[R.first + i];
	}
	if (tid == 0) {
		const u32 start = (u32)(R.out_off - R.low);
		run_len[r] = nok ? P.pos[R.first + nok - 1] + P.mlen[R.first + nok - 1] - start : 0;
		status[r] = nok == R.count                         ? (u32)ST_OK
			    : P.pos[R.first + nok] == LZ4P_NONE ? P.mst[R.first + nok]
								: (u32)ST_BAD_BLOCK;
	}
}

#endif
