/*
 * brotli_dec4_body.h -- the kernel of brotli_dec4.hip, which includes it once per B4_MODE with B4_NAME set: the same text
 * makes zmt_brotli_dec4_kernel (B4_RECORDS), the record pass of gpumt_brotli_decompress_batch_par (B4_WANTED) and its
 * execute stage (B4_SPANS).  Not a header of its own: no include guard, everything it defines it undefines.
 */
extern "C" __global__ void __launch_bounds__(64) B4_OCC
#if B4_MODE == B4_SPANS
B4_NAME(const u8 *__restrict__ stream, const B4Span *__restrict__ spans, u32 nrec, u8 *out_base, u32 *__restrict__ status)
#else
B4_NAME(const u8 *__restrict__ stream, const u64 *__restrict__ rec_off, const u32 *__restrict__ rec_len,
	u32 nrec, u8 *out_base, const u64 *__restrict__ out_off, const u32 *__restrict__ out_cap,
	u32 *__restrict__ out_len, u32 *__restrict__ status
#if B4_MODE == B4_WANTED
	, u32 want
#endif
	)
#endif
{
	__shared__ __attribute__((aligned(16))) B4Lds L;
#if B4_MODE == B4_SPANS
#define B4_SRC(u) spans[u].src
#define B4_SLEN(u) spans[u].src_len
#define B4_OUT(u) spans[u].out
#define B4_CAP(u) spans[u].out_len
#else
#define B4_SRC(u) rec_off[u]
#define B4_SLEN(u) rec_len[u]
#define B4_OUT(u) out_off[u]
#define B4_CAP(u) out_cap[u]
#endif
#if B4_MODE == B4_WANTED
#define B4_IS_WANTED(u) (status[u] == want)
#else
#define B4_IS_WANTED(u) true
#endif
#if B4_MODE == B4_SPANS
#define B4_FLAGS(u) spans[u].flags
#else
#define B4_FLAGS(u) B4_SPAN_FIRST
#endif
	const int lane = wv_lane();
	const u32 grp = (u32)lane >> 4, l16 = (u32)lane & 15u;
	if (lane < 24) {
		L.kins[lane] = (u32)BR_INS_BASE[lane] | (u32)BR_INS_BITS[lane] << 24;
		L.kcopy[lane] = (u32)BR_COPY_BASE[lane] | (u32)BR_COPY_BITS[lane] << 24;
	}
	wv_sync();
	/* this group's tree records, direct tables and window */
	const u32 gi = grp < B4_NG ? grp : 0u; /* (lanes of groups not in use idle; their pointers stay valid) */
	const u8 *const lit_rec = L.lit[gi];
	const u8 *const cmd_rec = L.cmd[gi];
	const u8 *const dist_rec = L.dist[gi];
	const u16 *const tab_lit = L.tab[gi][B4_T_LIT], *const tab_cmd = L.tab[gi][B4_T_CMD], *const tab_dist = L.tab[gi][B4_T_DIST];
	u8 *const win = L.win[gi];

	const u32 rec = blockIdx.x * B4_NG + grp;
	const bool exists = grp < B4_NG && rec < nrec && B4_IS_WANTED(rec);
	const u8 *const sp = stream + (exists ? B4_SRC(rec) : 0);
	const u32 slen = exists ? B4_SLEN(rec) : 0;
	u8 *const out = out_base + (exists ? B4_OUT(rec) : 0);
	const u32 cap = exists ? B4_CAP(rec) : 0;
	const u32 sflags = exists ? B4_FLAGS(rec) : B4_SPAN_FIRST;

	/* ---- per-stream state, the same in the 16 lanes of a group ---- */
	u32 st = exists ? B4_S_HDR : B4_S_DONE;
	u32 stc = ST_OK;
	u32 bitpos = 0; /* valid in B4_S_HDR / B4_S_FIN; while decoding the position is 8 * wptr - navail */
	/* bit buffer: acc holds the next navail (33..64) bits of the stream, nextw the dword behind them (stream byte wptr),
	 * read from the window [wbyte, wbyte + 264) a refill ahead */
	u64 acc = 0;
	u32 navail = 0, wptr = 0, nextw = 0, wbyte = 0;
	bool primed = false; /* the bit buffer is set up for the meta-block being decoded */
	u32 pos = 0, left = 0;
	bool first = (sflags & B4_SPAN_FIRST) != 0, was_last = false;
	u32 max_backward = first ? 0u : (1u << ((sflags >> 8) & 31u)) - 16u, npostfix = 0, ndirect = 0;
	u32 rb0 = 16, rb1 = 15, rb2 = 11, rb3 = 4; /* rb3 = last distance */
	u32 nring = first ? 4u : 0u; /* B4_SPANS: ring entries, newest first, that this span may read -- the ones it wrote */
	u32 lva = 0, lvi = 0, cva = 0, cvi = 0, dva = 0, dvi = 0;
	u32 bm_pos = 0, bm_dist = 0, bm_len = 0, nbatch = 0; /* lane j of the group: pending copy j */
	if (exists && slen >= (1u << 28)) { /* 32-bit bit positions */
		stc = B4_HANDOFF;
		st = B4_S_FIN;
	}

	/* window = stream bytes [W, W + 264), W a multiple of 4 (a damaged stream may run far past its end inside a
	 * meta-block: beyond the record + most of the stream's 256-byte slack the window reads as zeros, never from memory) */
#define B4_LOAD_WIN(W)                                                                                             \
	do {                                                                                                       \
		wbyte = (W);                                                                                       \
		const u32 o_ = wbyte + 16u * l16;                                                                  \
		u64 a_ = 0, b_ = 0, c_ = 0;                                                                        \
		if (o_ + 16u <= slen + 240u) {                                                                     \
			a_ = ld64u(sp + o_);                                                                       \
			b_ = ld64u(sp + o_ + 8);                                                                   \
		}                                                                                                  \
		*(u64 *)(win + 16u * l16) = a_;                                                                    \
		*(u64 *)(win + 16u * l16 + 8) = b_;                                                                \
		if (l16 == 0) {                                                                                    \
			if (wbyte + B4_WIN + 8u <= slen + 240u)                                                    \
				c_ = ld64u(sp + wbyte + B4_WIN);                                                   \
			*(u64 *)(win + B4_WIN) = c_;                                                               \
		}                                                                                                  \
		grp_sync();                                                                                        \
	} while (0)
	/* the next MARGIN stream bytes behind nextw must be in the window */
#define B4_ENSURE(cond, MARGIN)                                                                                    \
	do {                                                                                                       \
		const bool need_ = (cond) && (wptr - wbyte > B4_WIN - (MARGIN));                                   \
		if (wv_any(need_)) { /* (every group with `cond` reloads: one memory round trip for the wave, not one per group) */ \
			if (cond)                                                                                  \
				B4_LOAD_WIN(wptr);                                                                 \
		}                                                                                                  \
	} while (0)
	/* drop n (<= 24) bits; top the buffer up from nextw when 32 or fewer are left, and read the dword behind it */
#define B4_CONSUME(n)                                                                                              \
	do {                                                                                                       \
		acc >>= (n);                                                                                       \
		navail -= (n);                                                                                     \
		const bool rf_ = navail <= 32u;                                                                    \
		acc |= rf_ ? (u64)nextw << (navail & 63u) : 0ull;                                                  \
		navail += rf_ ? 32u : 0u;                                                                          \
		wptr += rf_ ? 4u : 0u;                                                                             \
		nextw = *(const u32 *)(win + (wptr - wbyte));                                                      \
	} while (0)
	/* next symbol of a tree, not consumed yet: direct table first (codes of <= 8 bits: one LDS read), the canonical walk
	 * otherwise.  PAY = the symbol's payload, LEN = its code length */
#define B4_SYMLEN(cond, TAB, REC, VA, VI, SYM16, PAY, LEN)                                                         \
	do {                                                                                                       \
		u32 e_ = (cond) ? (u32)(TAB)[(u32)acc & 255u] : 0x1000u;                                           \
		if (wv_any((cond) && (e_ >> 12) == 0)) {                                                           \
			if ((cond) && (e_ >> 12) == 0) {                                                           \
				u32 len_;                                                                          \
				const u32 k_ = b4_sym_index((u32)acc, VA, VI, &len_, hbad);                        \
				const u32 s_ = (SYM16) ? (u32) * (const u16 *)((REC) + 128 + 2 * (k_ & 1023u))     \
						       : (u32)(REC)[128 + (k_ & 255u)];                            \
				e_ = (s_ & 0xFFFu) | (len_ + 1u) << 12;                                            \
			}                                                                                          \
		}                                                                                                  \
		PAY = e_ & 0xFFFu;                                                                                 \
		LEN = (e_ >> 12) - 1u;                                                                             \
	} while (0)
#define B4_SYMBOL(cond, TAB, REC, VA, VI, SYM16, PAY)                                                              \
	do {                                                                                                       \
		u32 l_;                                                                                            \
		B4_SYMLEN(cond, TAB, REC, VA, VI, SYM16, PAY, l_);                                                 \
		if (cond)                                                                                          \
			B4_CONSUME(l_);                                                                            \
	} while (0)
	/* pending copies of the groups with `cond`: every lane its own copy once its source lies below the watermark (the
	 * destination of the group's first unfinished copy), long ones by the group together */
#define B4_EXEC(cond)                                                                                              \
	do {                                                                                                       \
		const bool ex_ = (cond) && nbatch != 0;                                                            \
		if (wv_any(ex_)) {                                                                                 \
			wave_mem_fence();                                                                          \
			if (ex_) {                                                                                 \
				const bool act_ = l16 < nbatch;                                                    \
				const u32 ml_ = act_ ? bm_len : 0;                                                 \
				const u32 src_ = bm_pos - bm_dist, eff_ = ml_ < bm_dist ? ml_ : bm_dist;           \
				bool fin_ = !act_;                                                                 \
				for (;;) {                                                                         \
					const u32 unf_ = grp_ballot(!fin_);                                        \
					if (!unf_)                                                                 \
						break;                                                             \
					const int fst_ = wv_ffs((u64)unf_) - 1;                                    \
					const u32 W_ = grp_shfl(bm_pos, fst_), hl_ = grp_shfl(ml_, fst_);          \
					if (hl_ > BR_CAP) {                                                        \
						b4_grp_match(out + W_, grp_shfl(bm_dist, fst_), hl_, l16);         \
						if ((int)l16 == fst_)                                              \
							fin_ = true;                                               \
					} else {                                                                   \
						const bool rdy_ = !fin_ && ml_ <= BR_CAP && src_ + eff_ <= W_;     \
						if (rdy_) {                                                        \
							g_match(out + bm_pos, bm_dist, ml_);                       \
							fin_ = true;                                               \
						}                                                                  \
					}                                                                          \
					b4_grp_fence();                                                            \
				}                                                                                  \
				nbatch = 0;                                                                        \
			}                                                                                          \
		}                                                                                                  \
	} while (0)

	for (;;) {
		/* ================= headers: wave-cooperative, one group at a time ================= */
		for (u32 g = 0; g < B4_NG; g++) {
			if (wv_readlane(st, (int)(16u * g)) != B4_S_HDR)
				continue;
			const int gl = (int)(16u * g);
			const bool mine = grp == g;
			BrBits b;
			{
				const u32 r_ = blockIdx.x * B4_NG + g;
				b.p = stream + B4_SRC(r_);
				b.n = wv_readfirst(B4_SLEN(r_));
			}
			const u32 g_cap = wv_readlane(cap, gl);
			const u32 bp = wv_readlane(bitpos, gl);
			u32 g_pos = wv_readlane(pos, gl);
			u8 *const g_out = out_base + B4_OUT(blockIdx.x * B4_NG + g);
			br_seek(b, bp >> 3, lane);
			if (bp & 7u)
				(void)br_get(b, bp & 7u, lane);
			u32 g_stc = ST_OK, g_st = B4_S_HDR;
			u32 g_left = 0, g_npostfix = 0, g_ndirect = 0, g_maxb = wv_readlane(max_backward, gl);
			bool g_last = wv_readlane((u32)was_last, gl) != 0;
			if (wv_readlane((u32)first, gl)) {
				/* 9.1 window bits */
				u32 wbits = 16;
				if (br_get(b, 1, lane)) {
					u32 v = br_get(b, 3, lane);
					if (v) {
						wbits = 17 + v;
					} else {
						v = br_get(b, 3, lane);
						if (v == 1)
							g_stc = BRBAD(); /* large-window streams are not brotli-mt's */
						wbits = v ? 8 + v : 17;
					}
				}
				g_maxb = (1u << wbits) - 16u;
			}
			while (g_stc == ST_OK && g_st == B4_S_HDR) {
				if (g_last) { /* the last meta-block is done: zero padding up to the byte boundary, nothing after counts */
					g_st = B4_S_FIN;
					break;
				}
				if (B4_MODE == B4_SPANS && br_used(b) == 8ull * b.n) { /* the span ends here, on a meta-block boundary */
					g_st = B4_S_FIN;
					break;
				}
				if (br_over(b)) {
					g_stc = BRBAD();
					break;
				}
				const u32 is_last = br_get(b, 1, lane);
				if (B4_MODE == B4_SPANS && is_last) { /* the stream's end is not a span's */
					g_stc = B4_HANDOFF;
					break;
				}
				if (is_last && br_get(b, 1, lane)) { /* ISLASTEMPTY */
					g_last = true;
					continue;
				}
				const u32 nib = br_get(b, 2, lane);
				if (nib == 3) {
					/* metadata meta-block: skipped */
					if (br_get(b, 1, lane)) {
						g_stc = BRBAD();
						break;
					}
					const u32 nb = br_get(b, 2, lane);
					u32 skip = 0;
					bool e = false;
					for (u32 i = 0; i < nb; i++) {
						const u32 v = br_get(b, 8, lane);
						if (i + 1 == nb && nb > 1 && v == 0)
							e = true;
						skip |= v << (8 * i);
					}
					if (nb)
						skip++;
					if ((br_used(b) & 7) && br_get(b, 8 - (u32)(br_used(b) & 7), lane))
						e = true;
					const u64 at = br_used(b) >> 3;
					if (e || br_over(b) || at + skip > b.n) {
						g_stc = BRBAD();
						break;
					}
					br_seek(b, (u32)at + skip, lane);
					if (is_last)
						g_last = true;
					continue;
				}
				u32 mlen = 0;
				{
					bool e = false;
					for (u32 i = 0; i < nib + 4; i++) {
						const u32 v = br_get(b, 4, lane);
						if (i + 1 == nib + 4 && nib && v == 0)
							e = true;
						mlen |= v << (4 * i);
					}
					if (e) {
						g_stc = BRBAD();
						break;
					}
				}
				mlen++;
				if (!is_last && br_get(b, 1, lane)) {
					/* uncompressed meta-block (pending copies read nothing it writes and it reads nothing at all) */
					if ((br_used(b) & 7) && br_get(b, 8 - (u32)(br_used(b) & 7), lane)) {
						g_stc = BRBAD();
						break;
					}
					const u64 at = br_used(b) >> 3;
					if (br_over(b) || at + mlen > b.n) {
						g_stc = BRBAD();
						break;
					}
					if (mlen > g_cap - g_pos) {
						g_stc = ST_SIZE_MISMATCH;
						break;
					}
					wave_copy(g_out + g_pos, b.p + at, mlen, lane);
					wave_mem_fence();
					g_pos += mlen;
					br_seek(b, (u32)at + mlen, lane);
					continue;
				}
				/* ---------------- compressed meta-block header (9.2): the simple shape only ---------------- */
				bool simple = true;
				for (u32 k = 0; k < 3 && simple; k++)
					simple = br_varlen8(b, lane) == 0; /* NBLTYPES == 1: no block-switch codes follow */
				if (!simple) {
					g_stc = B4_HANDOFF;
					break;
				}
				g_npostfix = br_get(b, 2, lane);
				g_ndirect = br_get(b, 4, lane) << g_npostfix;
				(void)br_get(b, 2, lane);                          /* context mode of the one literal block type */
				if (br_varlen8(b, lane) != 0 || br_varlen8(b, lane) != 0) { /* NTREESL, NTREESD: context maps */
					g_stc = B4_HANDOFF;
					break;
				}
				if (br_over(b)) {
					g_stc = BRBAD();
					break;
				}
				const u32 dist_alphabet = 16 + g_ndirect + (48u << g_npostfix);
				if (dist_alphabet > B4_DIST_MAX) {
					g_stc = B4_HANDOFF;
					break;
				}
				u8 *const g_lit = L.lit[g], *const g_cmd = L.cmd[g], *const g_dist = L.dist[g];
				bool bad = !br_read_code(b, L, g_lit, 256, false, lane) || br_over(b);
				if (!bad) {
					bad = !br_read_code(b, L, g_cmd, 704, true, lane) || br_over(b);
					/* insert&copy symbol -> insert code | copy code << 5 | "distance is the last one" << 10
					 * (RFC 7932 section 5; as in brotli_dec.hip) */
					u16 *sy = (u16 *)(g_cmd + 128);
					for (u32 k = (u32)lane; k < 704; k += 64) {
						const u32 v = sy[k];
						if (v < 704) {
							const u32 cell = v >> 6;
							const u32 icode = (((0x298500u >> (2 * cell)) & 3u) << 3) + ((v >> 3) & 7);
							const u32 ccode = (((0x262444u >> (2 * cell)) & 3u) << 3) + (v & 7);
							sy[k] = (u16)(icode | ccode << 5 | (v < 128 ? 1u << 10 : 0u));
						}
					}
					wv_sync();
				}
				if (!bad)
					bad = !br_read_code(b, L, g_dist, dist_alphabet, true, lane) || br_over(b);
				if (bad) {
					g_stc = BRBAD();
					break;
				}
				if (mlen > g_cap - g_pos) {
					g_stc = ST_SIZE_MISMATCH;
					break;
				}
				wv_sync();
				b4_build_tab(g_lit, L.tab[g][B4_T_LIT], false, lane);
				b4_build_tab(g_cmd, L.tab[g][B4_T_CMD], true, lane);
				b4_build_tab(g_dist, L.tab[g][B4_T_DIST], true, lane);
				g_left = mlen;
				g_last = is_last != 0;
				g_st = B4_S_DEC;
			}
			if (g_stc == ST_OK && g_st == B4_S_FIN) {
				if ((br_used(b) & 7) && br_get(b, 8 - (u32)(br_used(b) & 7), lane))
					g_stc = BRBAD();
				if (br_over(b))
					g_stc = BRBAD();
			}
			if (g_stc != ST_OK)
				g_st = B4_S_FIN;
			const u64 used = br_used(b);
			wv_sync();
			if (mine) {
				st = g_st;
				stc = g_stc;
				bitpos = (u32)used;
				primed = false;
				pos = g_pos;
				left = g_left;
				first = false;
				was_last = g_last;
				max_backward = g_maxb;
				npostfix = g_npostfix;
				ndirect = g_ndirect;
				if (g_st == B4_S_DEC) {
					const u64 el = *(const u64 *)(lit_rec + 8u * l16);
					const u64 ec = *(const u64 *)(cmd_rec + 8u * l16);
					const u64 ed = *(const u64 *)(dist_rec + 8u * l16);
					lva = (u32)el;
					lvi = (u32)(el >> 32);
					cva = (u32)ec;
					cvi = (u32)(ec >> 32);
					dva = (u32)ed;
					dvi = (u32)(ed >> 32);
				}
			}
		}
		/* ================= finished streams: pending copies, status ================= */
		if (wv_any(st == B4_S_FIN)) {
			B4_EXEC(st == B4_S_FIN && stc == ST_OK);
			wave_mem_fence();
			if (st == B4_S_FIN) {
				if (l16 == 0) {
#if B4_MODE == B4_SPANS
					status[rec] = stc == ST_OK && pos != cap ? ST_SIZE_MISMATCH : stc;
#else
					status[rec] = stc;
					out_len[rec] = stc == ST_OK ? pos : 0;
#endif
				}
				st = B4_S_DONE;
			}
		}
		if (!wv_any(st != B4_S_DONE))
			break;
		/* ================= bit buffers of the groups that start a meta-block ================= */
		if (wv_any(st == B4_S_DEC && !primed)) {
			if (st == B4_S_DEC && !primed) {
				B4_LOAD_WIN((bitpos >> 3) & ~3u);
				const u32 sh = bitpos - 8u * wbyte; /* 0..31 */
				const u32 w0 = *(const u32 *)win, w1 = *(const u32 *)(win + 4);
				acc = (((u64)w1 << 32) | w0) >> sh;
				navail = 64u - sh;
				wptr = wbyte + 8u;
				nextw = *(const u32 *)(win + 8);
				primed = true;
			}
		}
		/* ================= commands (section 10): the groups in lockstep, one command each per pass ================= */
		bool moved = !wv_any(st == B4_S_DEC) || wv_any(st == B4_S_HDR || st == B4_S_FIN); /* a group left B4_S_DEC: headers / status first */
		while (!moved) {
			const bool act = st == B4_S_DEC;
			bool hbad = false;
			u32 ins = 0, copy = 0;
			bool last_dist = false;
			B4_ENSURE(act, 40u); /* a command's own fields refill at most five times */
			{
				/* ---- insert&copy symbol, the extra bits of both lengths ---- */
				u32 cs, clen;
				B4_SYMLEN(act, tab_cmd, cmd_rec, cva, cvi, true, cs, clen);
				u32 ki = 0, kc = 0;
				bool wide = false;
				if (act) {
					const u32 icode = cs & 31u, ccode = (cs >> 5) & 31u;
					last_dist = (cs >> 10) & 1u;
					ki = L.kins[icode < 24u ? icode : 0u];
					kc = L.kcopy[ccode < 24u ? ccode : 0u];
					const u32 ib = ki >> 24, cb = kc >> 24; /* at most 24 bits each */
					const u32 tot = clen + ib + cb;
					wide = tot > 32u;
					if (!wide) {
						/* symbol and both extra fields inside the low word (nearly always): one step of the bit buffer */
						const u32 x = (u32)acc >> clen;
						ins = (ki & 0xFFFFFFu) + (x & ((1u << ib) - 1u));
						copy = (kc & 0xFFFFFFu) + ((x >> ib) & ((1u << cb) - 1u));
						B4_CONSUME(tot);
					}
				}
				if (wv_any(wide)) {
					if (wide) {
						const u32 ib = ki >> 24, cb = kc >> 24;
						B4_CONSUME(clen);
						ins = (ki & 0xFFFFFFu) + ((u32)acc & ((1u << ib) - 1u));
						B4_CONSUME(ib);
						copy = (kc & 0xFFFFFFu) + ((u32)acc & ((1u << cb) - 1u));
						B4_CONSUME(cb);
					}
				}
				if (act && ins > left)
					hbad = true;
			}
			/* ---- literals: max(insert lengths) passes, a group without literals left idles ---- */
			u32 todo = (act && !hbad) ? ins : 0;
			if (act && !hbad)
				left -= ins;
			while (wv_any(todo != 0)) {
				/* two literals per pass: the second one's table entry is read behind the first one's code length; a
				 * code of more than 8 bits (rare) sends the pass through the general symbol path, one literal */
				const bool la = todo != 0;
				B4_ENSURE(la, 12u);
				const bool two = todo >= 2u;
				/* (both table reads unconditional -- a group without literals left reads an entry it does not use -- and the
				 * pair stored by the group's first two lanes in one instruction: no exec-mask region on the pass's chain) */
				const u32 e0 = (u32)tab_lit[(u32)acc & 255u];
				const u32 l0 = ((e0 >> 12) - 1u) & 15u;
				const u32 e1 = (u32)tab_lit[(u32)(acc >> l0) & 255u];
				if (wv_any(la && ((e0 >> 12) == 0 || (two && (e1 >> 12) == 0)))) {
					u32 sym;
					B4_SYMBOL(la, tab_lit, lit_rec, lva, lvi, false, sym);
					if (la) {
						if (l16 == 0)
							out[pos] = (u8)sym;
						pos++;
						todo--;
						if (hbad)
							todo = 0;
					}
				} else if (la) {
					const u32 adv = two ? 2u : 1u;
					const u32 l1 = two ? (e1 >> 12) - 1u : 0u;
					if (l16 < adv)
						out[pos + l16] = (u8)(l16 ? e1 : e0);
					pos += adv;
					todo -= adv;
					B4_CONSUME(l0 + l1);
				}
			}
			/* ---- distance (section 4), the copy goes to the group's batch ---- */
			const bool dact = act && !hbad && left != 0;
			const bool dsym = dact && !last_dist;
			/* (the window margin left by the command's and the literal loop's checks covers the distance's two refills) */
			bool handoff = false;
			u32 dc, dlen;
			B4_SYMLEN(dsym, tab_dist, dist_rec, dva, dvi, true, dc, dlen);
			if (dact) {
				u32 dist = rb3;
				bool push = false;
				bool stale = B4_MODE == B4_SPANS && last_dist && nring == 0; /* a ring entry from before the span */
				if (!last_dist) {
					push = true;
					if (dc < 16u) {
						B4_CONSUME(dlen);
						const u32 which = dc < 4u ? dc : dc < 10u ? 0u : 1u;
						if (B4_MODE == B4_SPANS && which >= nring)
							stale = true;
						const u32 r = which == 0 ? rb3 : which == 1 ? rb2 : which == 2 ? rb1 : rb0;
						int del = 0;
						if (dc >= 4u) {
							const u32 q = (dc - 4u) % 6u; /* -1 +1 -2 +2 -3 +3 */
							del = (int)(q / 2u + 1u);
							if (!(q & 1u))
								del = -del;
						}
						const int dd = (int)r + del;
						if (dd <= 0)
							hbad = true;
						dist = (u32)dd;
						push = dc != 0;
					} else if (dc < 16u + ndirect) {
						B4_CONSUME(dlen);
						dist = dc - 15u;
					} else {
						/* (at most B4_DIST_MAX symbols: hcode < 48, nbits <= 24, the distance below 2^28 -- 32-bit arithmetic) */
						const u32 d = dc - ndirect - 16u;
						const u32 hcode = d >> npostfix, lcode = d & ((1u << npostfix) - 1u);
						u32 nbits = (1u + (hcode >> 1)) & 31u;
						if (nbits > 24u) {
							hbad = true;
							nbits = 0;
						}
						const u32 offset = ((2u + (hcode & 1u)) << nbits) - 4u;
						u32 xb;
						if (dlen + nbits <= 32u) { /* the symbol and its extra bits in one step of the bit buffer (nearly always) */
							xb = (u32)(acc >> dlen) & ((1u << nbits) - 1u);
							B4_CONSUME(dlen + nbits);
						} else {
							B4_CONSUME(dlen);
							xb = (u32)acc & ((1u << nbits) - 1u);
							B4_CONSUME(nbits);
						}
						dist = ((offset + xb) << npostfix) + lcode + ndirect + 1u;
					}
				}
				const u32 max_dist = pos < max_backward ? pos : max_backward;
				if (!hbad) {
					if (dist > max_dist || (B4_MODE == B4_SPANS && stale)) {
						handoff = true; /* static dictionary reference: the general kernel's (a span: a source before it) */
					} else if (copy > left) {
						hbad = true;
					} else {
						if (push) {
							rb0 = rb1;
							rb1 = rb2;
							rb2 = rb3;
							rb3 = dist;
							if (B4_MODE == B4_SPANS && nring < 4u)
								nring++;
						}
						if (l16 == nbatch) {
							bm_pos = pos;
							bm_dist = dist;
							bm_len = copy;
						}
						nbatch++;
						pos += copy;
						left -= copy;
					}
				}
			}
			/* (as soon as one group's 16 slots are full every group runs what it has pending: one fence and one memory
			 * round trip for the wave instead of one per group -- the groups fill their slots a pass or two apart) */
			if (wv_any(act && nbatch == B4_NB))
				B4_EXEC(act);
			if (act) {
				const u64 used = 8ull * wptr - navail;
				if (handoff) {
					stc = B4_HANDOFF;
					st = B4_S_FIN;
				} else if (hbad || (left == 0 && used > 8ull * slen)) {
					/* (a truncated stream shows at the end of the meta-block: the loop is bounded by MLEN) */
					stc = BRBAD();
					st = B4_S_FIN;
				} else if (left == 0) {
					bitpos = (u32)used;
					st = B4_S_HDR;
				}
			}
			moved = wv_any(st != B4_S_DEC && act);
		}
	}
#undef B4_LOAD_WIN
#undef B4_ENSURE
#undef B4_CONSUME
#undef B4_SYMBOL
#undef B4_EXEC
#undef B4_SRC
#undef B4_SLEN
#undef B4_OUT
#undef B4_CAP
#undef B4_IS_WANTED
#undef B4_FLAGS
}
#undef B4_MODE
#undef B4_NAME
