/*
 * zstd_dec_par.h -- the execute stage of a block run, block-parallel (gpumt_zstd_decompress_blocks_par); included by
 * zstd_dec.hip behind the entropy pre-pass, whose slots it reads, and the serial run decoder, whose results it reproduces.
 *
 * Behind the entropy pre-pass a marked block is a list of (ll, ml, offset value) and a literal buffer.  What it needs from
 * the blocks in front of it: three repeat offsets, its output position, and the bytes its matches read from before its
 * own start.  The first two are a scan over a few words per block; the third is lz4_dec_par.h's origin plane, here one
 * u32 per output byte (a zstd offset does not fit 16 bits): 0 = the value is there, p + 1 = the value is the byte at run
 * position p (positions count from the start of the run's history, 32 bits by hist + out_cap <= 0xFFFE0000).
 * No wave waits on another wave: the launches are stream-ordered, and resolve uses its workgroup's barrier.
 *
 *   plan      one wave: the runs of two or more blocks must lie in ascending, disjoint block ranges; owner[b] = run of b.
 *             Any other table decodes with the serial code, all of it.
 *   split     one wave per run: s = one past the last Compressed_Block that is not fully marked; [first, first + s) is the
 *             serial prefix, the rest the parallel suffix; a suffix of fewer than 2 blocks leaves the run serial.
 *   prefix    zstd_dec_body<RUN, PRE> over the derived prefix runs, on a scratch copy of the carry slot.
 *   measure   one wave per suffix block: decoded size, the checks that need no history, and the block's repeat-offset
 *             transfer function (z_rep_fold on tagged values: "incoming rep i minus d" or an absolute offset).
 *   scan      one wave per run: positions, incoming repeat offsets of every block, room.
 *   execute   one wave per suffix block at its final position; a match source inside another suffix block is not read,
 *             its position goes to the origin plane and travels with copies inside the block.
 *   resolve   one workgroup per run, blocks in order: out[p] = out[origin[p] - 1] wherever origin[p] != 0.
 *   fallback  one wave per run that is serial or that any stage refused: the serial RUN, PRE kernel over the caller's run
 *             record and untouched carry slot, so a failed run's verdict, length, bytes and carry are the serial ones.
 *   carry     one wave per good run: run_len, status, block_par, and the caller's carry slot (repeat offsets from scan,
 *             each table from its last definer in the suffix, else what the prefix or the incoming carry left).
 */
#ifndef ZMT_ZSTD_DEC_PAR_H
#define ZMT_ZSTD_DEC_PAR_H

#define ZPAR_NONE 0xFFFFFFFFu
#define ZPAR_UNRES 0x100u /* xst: the block left origins behind */
/* tagged repeat offsets of the transfer function: an offset is below 2^28 (offset codes above 27 are never marked), so
 * "incoming rep i" is (i + 1) << 30 | 2^29 and every `rep0 - 1` on it counts d down from there */
#define ZPAR_TAG(i) (((u32)(i) + 1u) << 30 | 0x20000000u)

/* scratch of one call: `origin` has one entry per byte of d_out, the other arrays one (or 3, 4) per run or per block */
struct ZPar {
	u32 *origin;
	ZRun *prun;  /* per run: the derived prefix run */
	u8 *pcarry;  /* per run: scratch copy of its carry slot */
	u32 *sfx;    /* per run: blocks of the serial prefix */
	u32 *rflag;  /* per run: 1 = serial or refused, decoded by the fallback kernel */
	u32 *plen, *pst; /* per run: length and status of the prefix */
	u32 *rrep;   /* per run x 3: repeat offsets behind the run */
	u32 *rlen;   /* per run: length of the run */
	u32 *rlast;  /* per run x 4: last definer of the Huffman / LL / OF / ML table (pre-pass resolve kernel) */
	u32 *owner;  /* per block: its run, ZPAR_NONE: of no run of two or more blocks (memset by the host) */
	u32 *blen;   /* per block: decoded size */
	u32 *bst;    /* per block: 0 = measured and clean */
	u32 *btf;    /* per block x 3: transfer function */
	u32 *bpos;   /* per block: position in the run's area */
	u32 *brep;   /* per block x 3: incoming repeat offsets */
	u32 *xst;    /* per block: verdict of execute | ZPAR_UNRES */
	u32 *flag;   /* [0] = the plan holds */
};

static __device__ __forceinline__ bool zpar_run_ok(const ZRun &R, u32 nblk, u64 out_bytes)
{
	return !(R.out_off > out_bytes || R.out_cap > out_bytes - R.out_off || R.hist > R.out_off ||
		 (u64)R.hist + R.out_cap > 0xFFFE0000ull || R.first > nblk || R.count > nblk - R.first || R.carry > 1);
}

static __device__ __forceinline__ bool zpar_block_ok(const ZBlock &B, u64 stream_bytes)
{
	return B.src_off <= stream_bytes && B.src_len <= stream_bytes - B.src_off && B.block_max <= Z_BLOCK_MAX && B.src_len >= 3;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_plan_kernel(const ZRun *__restrict__ runs, u32 nrun, u32 nblk, u64 out_bytes, ZPar P)
{
	const int lane = wv_lane();
	u32 hi = 0; /* end of the block ranges so far */
	bool bad = false;
	if (blockIdx.x != 0)
		return;
	for (int pass = 0; pass < 2; pass++) {
		if (pass && wv_any(bad))
			break;
		for (u32 base = 0; base < nrun; base += 64) {
			const u32 r = base + (u32)lane;
			u32 first = 0, count = 0;
			if (r < nrun) {
				const ZRun R = runs[r];
				if (zpar_run_ok(R, nblk, out_bytes) && R.count >= 2) {
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
zmt_zstd_par_split_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			  const ZRun *__restrict__ runs, u32 nrun, u64 out_bytes, const u32 *__restrict__ mark, ZPar P)
{
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (r >= nrun)
		return;
	const ZRun R = runs[r];
	u32 s = ZPAR_NONE;
	if (wv_readfirst(P.flag[0]) && zpar_run_ok(R, nblk, out_bytes) && R.count >= 2) {
		s = 0;
		for (u32 hi = R.count; hi > 0 && s == 0;) {
			const u32 n = hi < 64 ? hi : 64;
			bool need = false; /* a Compressed_Block without both mark bits */
			if ((u32)lane < n) {
				const u32 b = R.first + hi - 1 - (u32)lane;
				const ZBlock B = blocks[b];
				if (zpar_block_ok(B, stream_bytes))
					need = ((stream[B.src_off] >> 1) & 3) == 2 && mark[b] != (ZPRE_SEQ | ZPRE_LIT);
			}
			const u64 m = wv_ballot(need);
			if (m)
				s = hi - (u32)(wv_ffs(m) - 1);
			hi -= n;
		}
		if (R.count - s < 2)
			s = ZPAR_NONE;
	}
	if (lane == 0) {
		ZRun D = R;
		D.count = s == ZPAR_NONE ? 0 : s;
		D.flags = R.flags & ZR_FIRST; /* never the frame's last run: its state is wanted */
		P.prun[r] = D;
		P.sfx[r] = s;
		P.rflag[r] = s == ZPAR_NONE;
	}
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_prefix_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			   const ZRun *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes, const u8 *carry,
			   u8 *__restrict__ litbuf, const u32 *__restrict__ mark, const u32 *__restrict__ def,
			   const u8 *__restrict__ slots, ZPar P)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (r >= nrun || wv_readfirst(P.rflag[r]))
		return;
	const ZRun R = runs[r];
	if (!(R.flags & ZR_FIRST)) {
		const u32 *s = (const u32 *)(carry + (size_t)R.carry * sizeof(ZCarry));
		u32 *d = (u32 *)(P.pcarry + (size_t)r * sizeof(ZCarry));
		for (u32 i = (u32)lane; i < sizeof(ZCarry) / 4; i += 64)
			d[i] = s[i];
		wave_mem_fence();
	}
	zstd_dec_body<false, ZLds, true, true>(L, 0u, stream, stream_bytes, nullptr, nullptr, nrun, out_base, nullptr, P.plen,
					       litbuf, P.pst, nullptr, nullptr, nullptr, nullptr, 0, blocks, nblk, P.prun, out_bytes,
					       P.pcarry, mark, def, slots, true);
}

/* the suffix block b of run r, or false */
static __device__ __forceinline__ bool zpar_suffix_block(const ZPar &P, u32 b, const ZRun *__restrict__ runs, u32 &r, ZRun &R)
{
	if (!wv_readfirst(P.flag[0]))
		return false;
	r = wv_readfirst(P.owner[b]);
	if (r == ZPAR_NONE || wv_readfirst(P.rflag[r]))
		return false;
	R = runs[r];
	return b >= R.first + wv_readfirst(P.sfx[r]);
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_measure_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			    const ZRun *__restrict__ runs, const ZPre *__restrict__ pre, const u32 *__restrict__ mark,
			    const u8 *__restrict__ slots, ZPar P)
{
	const u32 b = blockIdx.x;
	const int lane = wv_lane();
	u32 r;
	ZRun R;
	if (b >= nblk || !zpar_suffix_block(P, b, runs, r, R))
		return;
	const ZBlock B = blocks[b];
	u32 bad = 1, len = 0, t0 = ZPAR_TAG(0), t1 = ZPAR_TAG(1), t2 = ZPAR_TAG(2);
	if (zpar_block_ok(B, stream_bytes)) {
		const u8 *h = stream + B.src_off;
		const u32 bh = uld8(h) | uld8(h + 1) << 8 | uld8(h + 2) << 16;
		const u32 btype = (bh >> 1) & 3, bsize = bh >> 3;
		if (btype == 0) {
			bad = bsize > B.block_max || B.src_len != 3 + bsize;
			len = bsize;
		} else if (btype == 1) {
			bad = bsize > B.block_max || B.src_len != 4;
			len = bsize;
		} else if (btype == 2 && wv_readfirst(mark[b]) == (ZPRE_SEQ | ZPRE_LIT)) {
			const ZPre Q = pre[b];
			const u32 nseq = wv_readfirst(Q.nseq), regen = wv_readfirst(Q.regen);
			const u64 *seq = (const u64 *)(slots + (size_t)b * Z_PRE_STRIDE + Z_PRE_LIT);
			u32 sll = 0, sml = 0;
			bad = !Q.ok || Q.bsize != B.src_len - 3 || bsize != Q.bsize || bsize > B.block_max || regen > B.block_max ||
			      nseq > Z_PRE_SEQCAP(B.block_max);
			for (u32 sbase = 0; sbase < nseq && !bad; sbase += 64) {
				const u32 k = nseq - sbase < 64 ? nseq - sbase : 64;
				const bool act0 = (u32)lane < k;
				u32 ll = 0, ml = 0, ofv = 4;
				if (act0) {
					const u64 v = seq[sbase + (u32)lane];
					ll = (u32)v & 0x3FFFFu;
					ml = (u32)(v >> 18) & 0x3FFFFu;
					ofv = (u32)(v >> 36);
				}
				u32 off = ofv - 3;
				if (wv_any(act0 && ofv == 0) || z_rep_fold(ofv, ll, act0, k, t0, t1, t2, off, lane))
					bad = 1; /* (an absolute 1 - 1: whatever comes in, the block fails) */
				sll += wv_readlane(wv_scan_incl(ll), 63);
				sml += wv_readlane(wv_scan_incl(ml), 63);
				if (sll > regen || sml > B.block_max)
					bad = 1;
			}
			len = regen + sml;
			if (len > B.block_max)
				bad = 1;
		}
	}
	if (lane == 0) {
		P.bst[b] = bad;
		P.blen[b] = len;
		P.btf[3 * (size_t)b] = t0;
		P.btf[3 * (size_t)b + 1] = t1;
		P.btf[3 * (size_t)b + 2] = t2;
	}
}

/* a transfer-function value over the incoming offsets; 0: the offset would be zero or below (a failure) */
static __device__ __forceinline__ u32 zpar_apply(u32 v, u32 r0, u32 r1, u32 r2)
{
	const u32 tag = v >> 30;
	if (!tag)
		return v;
	const u32 base = tag == 1 ? r0 : tag == 2 ? r1 : r2, d = 0x20000000u - (v & 0x3FFFFFFFu);
	return base > d ? base - d : 0u;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_scan_kernel(const ZRun *__restrict__ runs, u32 nrun, ZPar P)
{
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (r >= nrun || wv_readfirst(P.rflag[r]))
		return;
	const ZRun R = runs[r];
	const u32 s = wv_readfirst(P.sfx[r]), cap = R.hist + R.out_cap;
	const ZCarry *cy = (const ZCarry *)(P.pcarry + (size_t)r * sizeof(ZCarry));
	bool failed = wv_readfirst(P.pst[r]) != ST_OK;
	u32 at = R.hist + wv_readfirst(P.plen[r]);
	u32 r0 = wv_readfirst(cy->rep[0]), r1 = wv_readfirst(cy->rep[1]), r2 = wv_readfirst(cy->rep[2]);
	if (at > cap)
		failed = true;
	for (u32 base = s; base < R.count && !failed; base += 64) {
		const u32 i = base + (u32)lane, b = R.first + i;
		const bool act = i < R.count;
		u32 len = 0, f0 = ZPAR_TAG(0), f1 = ZPAR_TAG(1), f2 = ZPAR_TAG(2), bad = 0;
		if (act) {
			bad = P.bst[b];
			len = bad ? 0 : P.blen[b];
			f0 = P.btf[3 * (size_t)b];
			f1 = P.btf[3 * (size_t)b + 1];
			f2 = P.btf[3 * (size_t)b + 2];
		}
		const u32 inc = wv_scan_incl(len); /* 64 blocks of at most 128 KiB */
		const u32 p = at + (inc - len);
		if (wv_any(act && (bad || len > cap - at || inc > cap - at)))
			failed = true;
		/* the incoming offsets, block after block: three words a step */
		u32 i0 = 0, i1 = 0, i2 = 0;
		const u32 n = R.count - base < 64 ? R.count - base : 64;
		for (u32 j = 0; j < n && !failed; j++) {
			if ((u32)lane == j) {
				i0 = r0;
				i1 = r1;
				i2 = r2;
			}
			const u32 g0 = wv_readlane(f0, (int)j), g1 = wv_readlane(f1, (int)j), g2 = wv_readlane(f2, (int)j);
			const u32 n0 = zpar_apply(g0, r0, r1, r2), n1 = zpar_apply(g1, r0, r1, r2), n2 = zpar_apply(g2, r0, r1, r2);
			if (!n0 || !n1 || !n2)
				failed = true;
			r0 = n0;
			r1 = n1;
			r2 = n2;
		}
		if (act && !failed) {
			P.bpos[b] = p;
			P.brep[3 * (size_t)b] = i0;
			P.brep[3 * (size_t)b + 1] = i1;
			P.brep[3 * (size_t)b + 2] = i2;
		}
		at += wv_readlane(inc, 63);
	}
	if (lane == 0) {
		if (failed)
			P.rflag[r] = 1;
		P.rrep[3 * (size_t)r] = r0;
		P.rrep[3 * (size_t)r + 1] = r1;
		P.rrep[3 * (size_t)r + 2] = r2;
		P.rlen[r] = at - R.hist;
	}
}

/* one byte of a match whose source is not all of one kind: root = where the byte comes from (below the match) */
static __device__ __forceinline__ bool zpar_byte(u8 *out, u32 *org, u32 dst, u32 root, u32 pstart, u32 bstart)
{
	if (root < pstart) {
		out[dst] = out[root]; /* final in memory: history or the prefix */
	} else if (root >= bstart) {
		out[dst] = out[root]; /* the block's own: value and origin */
		org[dst] = org[root];
	} else {
		org[dst] = root + 1; /* another suffix block's: not read */
		return true;
	}
	return false;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_exec_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			 const ZRun *__restrict__ runs, const ZPre *__restrict__ pre, u8 *__restrict__ slots, u8 *out_base,
			 ZPar P)
{
	const u32 b = blockIdx.x;
	const int lane = wv_lane();
	u32 r;
	ZRun R;
	if (b >= nblk || !zpar_suffix_block(P, b, runs, r, R))
		return;
	/* plan, split, measure and scan have checked the entries: [bstart, bstart + blen) lies inside the run's area */
	const ZBlock B = blocks[b];
	const u32 bstart = wv_readfirst(P.bpos[b]), blen = wv_readfirst(P.blen[b]), bend = bstart + blen;
	const u32 pstart = R.hist + wv_readfirst(P.plen[r]);
	u8 *out = out_base + (R.out_off - R.hist);
	u32 *org = P.origin + (R.out_off - R.hist);
	const u8 *h = stream + B.src_off;
	const u32 bh = uld8(h) | uld8(h + 1) << 8 | uld8(h + 2) << 16;
	const u32 btype = (bh >> 1) & 3;
	u32 x = ST_OK;
	bool un = false;
	for (u32 i = (u32)lane; i < blen; i += 64)
		org[bstart + i] = 0;
	if (btype == 0) {
		wave_copy(out + bstart, h + 3, blen, lane);
	} else if (btype == 1) {
		const u8 v = (u8)uld8(h + 3);
		for (u32 i = (u32)lane; i < blen; i += 64)
			out[bstart + i] = v;
	} else {
		const ZPre Q = pre[b];
		const u32 nseq = wv_readfirst(Q.nseq), regen = wv_readfirst(Q.regen), ltype = wv_readfirst(Q.lit) & 3;
		u8 *slot = slots + (size_t)b * Z_PRE_STRIDE;
		const u64 *seq = (const u64 *)(slot + Z_PRE_LIT);
		const u8 *lit = slot;
		if (ltype == 0) {
			lit = h + 3 + (wv_readfirst(Q.lit) >> 8);
		} else if (ltype == 1) {
			const u8 v = (u8)uld8(h + 3 + (wv_readfirst(Q.lit) >> 8));
			for (u32 i = (u32)lane * 8; i < regen + 8; i += 512)
				st64g(slot + i, 0x0101010101010101ull * v);
		}
		wave_mem_fence();
		u32 rep0 = wv_readfirst(P.brep[3 * (size_t)b]), rep1 = wv_readfirst(P.brep[3 * (size_t)b + 1]),
		    rep2 = wv_readfirst(P.brep[3 * (size_t)b + 2]);
		u32 opos = bstart, lpos = 0;
		for (u32 sbase = 0; sbase < nseq && x == ST_OK; sbase += 64) {
			const u32 k = nseq - sbase < 64 ? nseq - sbase : 64;
			const bool act0 = (u32)lane < k;
			u32 ll = 0, ml = 0, ofv = 4;
			if (act0) {
				const u64 v = seq[sbase + (u32)lane];
				ll = (u32)v & 0x3FFFFu;
				ml = (u32)(v >> 18) & 0x3FFFFu;
				ofv = (u32)(v >> 36);
			}
			u32 off = ofv - 3;
			if (wv_any(act0 && ofv == 0) || z_rep_fold(ofv, ll, act0, k, rep0, rep1, rep2, off, lane)) {
				x = ZBAD(); /* (rep0 - 1 == 0 with the real incoming offsets) */
				break;
			}
			const u32 len = ll + ml;
			const u32 incl = wv_scan_incl(len), lincl = wv_scan_incl(ll);
			const u32 tot = wv_readlane(incl, 63), ltot = wv_readlane(lincl, 63);
			if (ltot > regen - lpos || tot > bend - opos) {
				x = ZBAD();
				break;
			}
			const u32 op = opos + incl - len, mpos = op + ll, lsrc = lpos + lincl - ll;
			if (wv_any(act0 && off > mpos)) {
				x = ZBAD(); /* reaches before the start of the history */
				break;
			}
			const u32 src_pos = mpos - off, eff = ml < off ? ml : off;
			/* where the source lies: final memory / this block / another suffix block / not all of one kind */
			const bool c_fin = src_pos + eff <= pstart, c_own = src_pos >= bstart;
			const bool c_oth = !c_fin && !c_own && src_pos >= pstart && src_pos + eff <= bstart;
			const bool c_mix = act0 && ml && !c_fin && !c_own && !c_oth;
			if (act0 && ll <= Z_CAP)
				g_copy(out + op, lit + lsrc, ll);
			{
				u64 m = wv_ballot(act0 && ll > Z_CAP);
				while (m) {
					const int j = wv_ffs(m) - 1;
					m &= m - 1;
					wave_copy(out + wv_readlane(op, j), lit + wv_readlane(lsrc, j), wv_readlane(ll, j), lane);
				}
			}
			bool fin = !act0 || ml == 0;
			/* another block's bytes: origins only, nothing is read, so no order either */
			if (!fin && c_oth) {
				if (ml <= Z_CAP)
					for (u32 i = 0; i < ml; i++)
						org[mpos + i] = src_pos + i % off + 1;
				un = true;
			}
			{
				u64 m = wv_ballot(!fin && c_oth && ml > Z_CAP);
				while (m) {
					const int j = wv_ffs(m) - 1;
					m &= m - 1;
					const u32 jm = wv_readlane(mpos, j), js = wv_readlane(src_pos, j), jo = wv_readlane(off, j),
						  jl = wv_readlane(ml, j);
					for (u32 i = (u32)lane; i < jl; i += 64)
						org[jm + i] = js + i % jo + 1;
				}
			}
			if (c_oth)
				fin = true;
			wave_mem_fence();
			/* matches: the watermark rounds of zstd_dec_body; W = everything below is written and visible */
			for (;;) {
				const u64 unf = wv_ballot(!fin);
				if (!unf)
					break;
				const int fst = wv_ffs(unf) - 1;
				const u32 W = wv_readlane(mpos, fst), wml = wv_readlane(ml, fst), woff = wv_readlane(off, fst);
				if (wv_readlane((u32)c_mix, fst)) {
					/* at the head of the queue everything below it is there: bytewise, whole wave */
					const u32 ws = wv_readlane(src_pos, fst);
					for (u32 i = (u32)lane; i < wml; i += 64)
						if (zpar_byte(out, org, W + i, ws + i % woff, pstart, bstart))
							un = true;
					if (lane == fst)
						fin = true;
				} else if (wml > Z_CAP) {
					wave_match(out + W, woff, wml, lane);
					if (wv_readlane((u32)c_own, fst))
						wave_match((u8 *)(org + W), 4 * woff, 4 * wml, lane);
					if (lane == fst)
						fin = true;
				} else {
					const bool ready = !fin && !c_mix && ml <= Z_CAP && src_pos + eff <= W;
					if (ready) {
						g_match(out + mpos, off, ml);
						if (c_own)
							g_match((u8 *)(org + mpos), 4 * off, 4 * ml);
						fin = true;
					}
				}
				wave_mem_fence();
			}
			opos += tot;
			lpos += ltot;
		}
		if (x == ST_OK) {
			const u32 restl = regen - lpos;
			if (restl != bend - opos)
				x = ZBAD(); /* (not what measure counted) */
			else
				wave_copy(out + opos, lit + lpos, restl, lane);
		}
	}
	un = wv_any(un);
	if (lane == 0) {
		P.xst[b] = x == ST_OK ? (un ? ZPAR_UNRES : 0u) : x;
		if (x != ST_OK)
			P.rflag[r] = 1; /* (every writer writes 1) */
	}
}

struct ZParQuad {
	u32 v[4];
};
#define ZPAR_RESOLVE_THREADS 1024
extern "C" __global__ void __launch_bounds__(ZPAR_RESOLVE_THREADS)
zmt_zstd_par_resolve_kernel(const ZRun *__restrict__ runs, u32 nrun, u8 *out_base, ZPar P)
{
	__shared__ u32 s_bad;
	const u32 r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
	if (r >= nrun || P.rflag[r])
		return;
	const ZRun R = runs[r];
	const u32 s = P.sfx[r];
	u8 *out = out_base + (R.out_off - R.hist);
	const u32 *org = P.origin + (R.out_off - R.hist);
	if (tid == 0)
		s_bad = 0;
	__syncthreads();
	for (u32 i = s; i < R.count; i++) {
		const u32 b = R.first + i;
		if (!(P.xst[b] & ZPAR_UNRES))
			continue; /* (the same for every thread) */
		const u32 S = P.bpos[b], L = P.blen[b], L4 = L & ~3u;
		bool bad = false;
		for (u32 j = tid * 4; j < L4; j += nt * 4) {
			ZParQuad q;
			__builtin_memcpy(&q, org + S + j, 16);
			if (!(q.v[0] | q.v[1] | q.v[2] | q.v[3]))
				continue;
			for (u32 k = 0; k < 4; k++) {
				const u32 o = q.v[k];
				if (o > S) /* an origin lies below its block's start */
					bad = true;
				else if (o)
					out[S + j + k] = out[o - 1];
			}
		}
		if (tid < L - L4) {
			const u32 o = org[S + L4 + tid];
			if (o > S)
				bad = true;
			else if (o)
				out[S + L4 + tid] = out[o - 1];
		}
		if (bad)
			s_bad = 1;
		/* block i is final before block i + 1 reads it */
#ifndef ZMT_EMU
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#endif
		__syncthreads();
#ifndef ZMT_EMU
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
	}
	__syncthreads();
	if (tid == 0 && s_bad)
		P.rflag[r] = 1;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_fallback_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			     const ZRun *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes, u8 *carry,
			     u32 *__restrict__ run_len, u32 *__restrict__ status, u8 *__restrict__ litbuf,
			     const u32 *__restrict__ mark, const u32 *__restrict__ def, const u8 *__restrict__ slots, ZPar P)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	if (blockIdx.x >= nrun || !wv_readfirst(P.rflag[blockIdx.x]))
		return;
	zstd_dec_body<false, ZLds, true, true>(L, 0u, stream, stream_bytes, nullptr, nullptr, nrun, out_base, nullptr, run_len,
					       litbuf, status, nullptr, nullptr, nullptr, nullptr, 0, blocks, nblk, runs, out_bytes,
					       carry, mark, def, slots);
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_par_carry_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			  const ZRun *__restrict__ runs, u32 nrun, const ZPre *__restrict__ pre, u8 *carry,
			  u32 *__restrict__ run_len, u32 *__restrict__ status, u32 *__restrict__ block_par, ZPar P)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (lane < 36)
		L.llx[lane] = Z_LL_BASE[lane] | (u32)Z_LL_BITS[lane] << 24;
	if (lane < 53)
		L.mlx[lane] = Z_ML_BASE[lane] | (u32)Z_ML_BITS[lane] << 24;
	if (r >= nrun || wv_readfirst(P.rflag[r]))
		return;
	const ZRun R = runs[r];
	const u32 s0 = R.first + wv_readfirst(P.sfx[r]); /* the first suffix block */
	for (u32 i = s0 + (u32)lane; i < R.first + R.count; i += 64)
		block_par[i] = 1;
	if (lane == 0) {
		run_len[r] = P.rlen[r];
		status[r] = ST_OK;
	}
	if (R.flags & ZR_LAST)
		return;
	const u8 *mem_lo = stream, *mem_hi = stream + stream_bytes + 256;
	ZCarry *cy = (ZCarry *)(P.pcarry + (size_t)r * sizeof(ZCarry));
	if (lane < 3)
		cy->rep[lane] = P.rrep[3 * (size_t)r + (u32)lane];
	if (lane == 0)
		cy->corrupt = 0;
	/* the Huffman table: the last block of the suffix that describes a tree (the steps of the entropy kernel) */
	const u32 dh = wv_readfirst(P.rlast[4 * (size_t)r]);
	if (dh != ZPAR_NONE && dh >= s0 && dh < R.first + R.count) {
		const ZPre T = pre[dh];
		const u8 *tsrc = stream + blocks[dh].src_off + 3;
		const u32 thl = T.lit >> 8;
		wv_sync();
		stage_load(L.stage, tsrc, 0, 256, 0, mem_lo, mem_hi, lane);
		wv_sync();
		if (lane == 0) {
			const u32 avail = T.lcsz < 256 - thl ? T.lcsz : 256 - thl;
			int nw = 0, lg = 0;
			const int used = huf_read_weights(L.stage + thl, avail, L.w, &nw, &lg, (u32 *)L.sq[0], L.norm[0], L.next[0]);
			L.misc[ZM_ERR] = used < 0 || lg > 11;
			L.misc[ZM_G] = (u32)nw;
			L.misc[ZM_H] = (u32)lg;
		}
		wv_sync();
		if (!L.misc[ZM_ERR]) { /* (a marked treeless block behind it, or the block itself, decoded with this tree) */
			const int huf_log = (int)L.misc[ZM_H];
			for (u32 i = (u32)lane; i < (1u << 11); i += 64)
				L.huf[i] = 0;
			wv_sync();
			huf_fill(L.huf, L.w, (int)L.misc[ZM_G], huf_log, lane);
			wv_sync();
			for (u32 i = (u32)lane; i < (1u << 11); i += 64)
				cy->huf[i] = L.huf[i];
			if (lane == 0) {
				cy->huf_ok = 1;
				cy->huf_log = (u32)huf_log;
			}
		}
	}
	/* LL, OF, ML: each from the last block of the suffix that describes it */
	for (int t = 0; t < 3; t++) {
		const u32 d = wv_readfirst(P.rlast[4 * (size_t)r + 1 + (u32)t]);
		if (d == ZPAR_NONE || d < s0 || d >= R.first + R.count)
			continue;
		const ZPre D = pre[d];
		if (!zpre_seq_header(L, stream + blocks[d].src_off + 3, D, 1u << t, mem_lo, mem_hi, lane))
			continue;
		u32 *cells = t == 0 ? L.ll : t == 1 ? L.of : L.ml;
		u32 *dst = t == 0 ? cy->ll : t == 1 ? cy->of : cy->ml;
		if (lane == t) {
			const u32 spec = L.misc[ZM_A + t];
			u32 ok = 1, lg = 0;
			if (spec == 0xFFFFFFFFu) {
				ok = 0;
			} else if (spec & 0x80000000u) {
				const u32 sy = spec & 255;
				cells[0] = sy | (t == 1 ? sy : (t == 0 ? L.llx[sy] : L.mlx[sy]) >> 24) << 10;
			} else {
				lg = (spec >> 8) & 255;
				ok = lg <= (t == 1 ? 8u : 9u) &&
				     fse_build(cells, L.norm[t], (int)(spec & 255), (int)lg, L.next[t],
					       t == 0 ? L.llx : t == 2 ? L.mlx : (const u32 *)nullptr, lane) == 0;
			}
			L.misc[ZM_ERR] = !ok;
			if (ok) {
				cy->tab_ok[t] = 1;
				cy->tab_log[t] = lg;
				cy->tab_pre[t] = (spec & 0xC0000000u) == 0x40000000u;
			}
			L.misc[ZM_F] = lg;
		}
		wv_sync();
		if (!L.misc[ZM_ERR])
			for (u32 i = (u32)lane; i < (1u << L.misc[ZM_F]); i += 64)
				dst[i] = cells[i];
		wv_sync();
	}
	wave_mem_fence();
	{
		const u32 *sp = (const u32 *)cy;
		u32 *dp = (u32 *)(carry + (size_t)R.carry * sizeof(ZCarry));
		for (u32 i = (u32)lane; i < sizeof(ZCarry) / 4; i += 64)
			dp[i] = sp[i];
	}
}

#endif
