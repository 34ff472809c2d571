/*
 * zstd_dec.hip -- zstd frame decoder for gfx950, one wave per record.
 *
 * Replaces ZSTD_decompressStream as called per record by the reference
 * (/root/reference/lib/zstd-mt_decompress.c:464, one frame per 12-byte skippable record, :300-369).
 * Format: RFC 8878 -- raw / RLE / compressed blocks, Huffman literals (direct or FSE-compressed
 * weights, 1 or 4 streams, treeless), FSE sequence tables (predefined / RLE / compressed /
 * repeat), repeat offsets.  No dictionaries.
 *
 * Work split inside the wave (the format is a chain of serial bitstreams, so lanes are used where
 * the format offers independent streams and for all byte moving):
 *   - every header / table description is staged into LDS with one coalesced load and parsed there;
 *   - Huffman literals: the 4 streams decode on 4 lanes from 256-byte LDS windows that the wave
 *     refills cooperatively every 128 symbols; decoded literals go to a per-record scratch in HBM;
 *   - FSE tables: the three tables of a block are built on three lanes at once;
 *   - sequences: lane 0 walks the FSE bitstream from a 1 KiB LDS window, 64 sequences at a time;
 *     the wave then executes the 64 sequences in parallel: prefix sums give output and literal
 *     positions, every lane copies its own literals and match (8-byte unaligned global accesses),
 *     matches that read this batch's own output resolve in watermark rounds, long copies are
 *     done by the whole wave;
 *   - units: a block with a Huffman tree (or raw literals) followed by blocks with treeless (raw)
 *     literals, all with the predefined sequence tables or all with the tables the first one
 *     describes (repeat mode) -- what the device encoder writes per 128 KiB -- is
 *     decoded side by side: up to 64 Huffman streams on 64 lanes, then up to 16 sequence
 *     bitstreams on 16 x (LL, OF, ML) lanes into the record's scratch; the blocks then only
 *     execute.  Anything else ends the unit and takes the per-block path above.
 */
#include "zstd_dec_common.h"
#include "zstd_dec_seq.h"

/* LDS of one wave.  Table capacities are template parameters: the format allows Huffman codes of up
 * to 11 bits and FSE tables of 2^9 / 2^8 / 2^9 cells (13 KiB per wave, 12 waves per CU), but frames
 * whose blocks stay within 10 bits and the predefined 2^6 / 2^5 / 2^6 tables -- everything the
 * device encoder writes -- fit in 6 KiB, i.e. the 16 waves per CU the register budget allows.  The
 * small variant runs first and hands records that exceed it to the general one. */
template <int HCAP, int LLCAP, int OFCAP, int MLCAP> struct ZLdsT {
	u16 huf[1 << HCAP];  /* sym | nbits << 8 */
	u32 ll[1 << LLCAP], of[1 << OFCAP], ml[1 << MLCAP]; /* FSE cells, see ZC_* */
	u8 below[16];   /* stage[-16..0): 8-byte reads may start below the window */
	u8 stage[Z_STAGE + 16];
	u64 sq[3][64]; /* one batch of sequences, per LL / OF / ML: extra bits | code << 32 */
	u8 w[256];
	short norm[3][64];
	u16 next[3][64];
	u32 llx[36], mlx[53]; /* value base | extra bits << 24 of every LL / ML code */
	u32 misc[16];
	static constexpr int hcap = HCAP, llcap = LLCAP, ofcap = OFCAP, mlcap = MLCAP;
};
typedef ZLdsT<11, 9, 8, 9> ZLds;      /* everything RFC 8878 allows */
typedef ZLdsT<11, 6, 5, 6> ZLdsSmall; /* predefined-size sequence tables (frames whose sequences the pre-pass decoded need none) */
static_assert(offsetof(ZLdsSmall, sq) - offsetof(ZLdsSmall, below) == 1056 &&
		      offsetof(ZLds, sq) - offsetof(ZLds, below) == 1056,
	      "below | stage | sq are one region (per-lane stream windows)");

enum { ZM_ERR = 0, ZM_A, ZM_B, ZM_C, ZM_D, ZM_E, ZM_F, ZM_G, ZM_H };

/* ------------------------------------------------------------------ block runs (gpumt_zstd_decompress_blocks)
 * A plain .zst frame larger than a batch is decoded run by run: the consecutive blocks of the frame that one batch holds,
 * one wave per run, started at a block header.  The caller has parsed the frame header and the block headers. */
struct ZBlock { /* == gpumt_zstd_block */
	u64 src_off; /* the 3-byte block header in the stream */
	u32 src_len; /* header + body */
	u32 block_max;
};
struct ZRun { /* == gpumt_zstd_run */
	u64 out_off;
	u32 out_cap, hist, first, count, flags, carry;
};
#define ZR_FIRST 1u /* the frame starts here: nothing is carried in */
#define ZR_LAST 2u  /* the frame ends here: nothing is carried out */
/* What a later block of a frame may refer to (RFC 8878 3.1.1.3.1.1 treeless literals, 3.1.1.3.2.1 Repeat_Mode, 3.1.1.5
 * repeat offsets), as the wave holds it when a run ends; `corrupt` fails the runs that follow a failed one. */
struct ZCarry { /* GPUMT_ZSTD_CARRY_BYTES */
	u32 rep[3], huf_ok, huf_log, tab_ok[3], tab_log[3], tab_pre[3], corrupt, pad;
	u16 huf[1 << 11];
	u32 ll[1 << 9], of[1 << 8], ml[1 << 9];
};
static_assert(sizeof(ZCarry) == 9280, "GPUMT_ZSTD_CARRY_BYTES in include/gpumt.h");
#define Z_RUN_LITSLOT (Z_BLOCK_MAX + 256u) /* literal scratch per run = GPUMT_ZSTD_RUN_SCRATCH */
/* The entropy pre-pass of a call's block table (gpumt_zstd_decompress_blocks_pre, the kernels at the end of this file): what
 * the classify kernel found in a block's headers, one record per block of the table ... */
struct ZPre {
	u32 ok;    /* a Compressed_Block whose three headers parse; 0: left to the serial path */
	u32 lit;   /* Literals_Block_Type | streams << 2 | bytes of the literals section header << 8 */
	u32 regen, lcsz; /* Regenerated_Size, Compressed_Size (= regen for raw, 1 for RLE literals) */
	u32 sq0;   /* the sequences section, from the start of the block's body */
	u32 nseq;
	u32 sqh;   /* bytes of Number_of_Sequences and the modes byte | Symbol_Compression_Modes << 8 */
	u32 bsize;
};
/* ... the block that defines each table it uses (resolve kernel: def[4 b + k], k = Huffman, LL, OF, ML; the block's own index
 * when it describes the table itself, ZPRE_NONE when no block of the same run in this call does), and its two slots: */
#define ZPRE_NONE 0xFFFFFFFFu
#define Z_PRE_SEQCAP(block_max) ((block_max) / 4u) /* sequences a block's slot holds; a denser block stays serial */
#define Z_PRE_LIT (Z_BLOCK_MAX + 256u)
#define Z_PRE_STRIDE (Z_PRE_LIT + 8u * Z_PRE_SEQCAP(Z_BLOCK_MAX)) /* literals | sequences = GPUMT_ZSTD_PRE_SCRATCH(128 KiB) */
#define ZPRE_SEQ 1u /* mark bits: the block's sequences are in its slot ... */
#define ZPRE_LIT 2u /* ... its literals are (or need no decoding: raw, RLE) */


/* ------------------------------------------------------------------ the kernel */
#ifdef ZMT_EMU
static inline u32 zbad_(int line)
{
	if (getenv("ZMT_EMU_DEBUG") && wv_lane() == 0)
		fprintf(stderr, "zstd_dec: bad block flagged at line %d\n", line);
	return ST_BAD_BLOCK;
}
#define ZBAD() zbad_(__LINE__)
#else
#define ZBAD() ST_BAD_BLOCK
#endif
#ifndef ZMT_EMU
#define ZT() (PROF ? (u64)clock64() : 0ull)
#else
#define ZT() 0ull
#endif
#define ZP(i)                                                                                      \
	do {                                                                                       \
		if (PROF) {                                                                        \
			const u64 t_ = ZT();                                                       \
			pc[PROF ? (i) : 0] += t_ - tq;                                             \
			tq = t_;                                                                   \
		}                                                                                  \
	} while (0)

/* Repeat offsets of one batch of k <= 64 sequences, one per lane (RFC 8878 3.1.1.5): `off` arrives as offset value - 3 and
 * leaves as the offset of the lane's sequence, rep0..2 as they stand behind the batch.  Runs of new offsets fold into the
 * history in one step, only the sequences that use a repeat code are walked one by one.  True: a repeat code gave offset 0. */
static __device__ __forceinline__ bool z_rep_fold(u32 ofv, u32 ll, bool act0, u32 k, u32 &rep0, u32 &rep1, u32 &rep2, u32 &off,
						   int lane)
{
	u64 repm = wv_ballot(act0 && ofv <= 3);
	u32 prev = 0;
	bool rerr = false;
	for (;;) {
		const u32 j = repm ? (u32)wv_ffs(repm) - 1 : k;
		const u32 m = j - prev;
		if (m >= 1) {
			const u32 o1 = wv_readlane(off, (int)(j - 1));
			u32 n1, n2;
			if (m >= 3) {
				n1 = wv_readlane(off, (int)(j - 2));
				n2 = wv_readlane(off, (int)(j - 3));
			} else if (m == 2) {
				n1 = wv_readlane(off, (int)(j - 2));
				n2 = rep0;
			} else {
				n1 = rep0;
				n2 = rep1;
			}
			rep2 = n2;
			rep1 = n1;
			rep0 = o1;
		}
		if (j >= k)
			break;
		const u32 idx = wv_readlane(ofv, (int)j) - 1 + (wv_readlane(ll, (int)j) == 0);
		u32 o = rep0;
		if (idx) {
			o = idx == 1 ? rep1 : idx == 2 ? rep2 : rep0 - 1;
			if (o == 0)
				rerr = true;
			if (idx > 1)
				rep2 = rep1;
			rep1 = rep0;
			rep0 = o;
		}
		if ((u32)lane == j)
			off = o;
		repm &= repm - 1;
		prev = j + 1;
	}
	return rerr;
}

/* RUN: the same decoder started at a block header instead of a frame header (zmt_zstd_dec_run_kernel, at the end of this
 * file): "record" rec is run rec of `runs`, its blocks are entries of `blocks`, out_len receives the run's length, and what
 * a frame's later blocks may refer to travels in a ZCarry.  No units and no pre-pass there: one block after the other. */
/* PRE (with RUN): the execute stage behind the entropy pre-pass.  A block whose mark the pre-pass set takes its literals and
 * its sequences from its slots instead of walking the Huffman and FSE bitstreams; its tables are still built here, block
 * after block, so what a later unmarked block refers to and what the carry receives are the serial decoder's by
 * construction.  A mark counts only if the definers the pre-pass used are the ones this wave arrived at itself. */
template <bool PROF, typename LDS, bool RUN = false, bool PRE = false>
static __device__ __forceinline__ void
zstd_dec_body(LDS &L, u32 want_status, const u8 *__restrict__ stream, u64 stream_bytes, const u64 *__restrict__ rec_off,
	      const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base, const u64 *__restrict__ out_off,
	      u32 *__restrict__ out_len, u8 *__restrict__ litbuf, u32 *__restrict__ status,
	      u32 *__restrict__ chk_expect, u32 *__restrict__ chk_valid, unsigned long long *prof, u8 *seqbuf, u64 seqcap,
	      const ZBlock *__restrict__ blocks = nullptr, u32 nblk = 0, const ZRun *__restrict__ runs = nullptr,
	      u64 out_bytes = 0, u8 *carry_base = nullptr, const u32 *__restrict__ pre_mark = nullptr,
	      const u32 *__restrict__ pre_def = nullptr, const u8 *__restrict__ pre_slots = nullptr, bool carry_by_rec = false)
{
	const int lane = wv_lane();
	u64 pc[PROF ? 8 : 1] = {0}, tq = ZT();
	const u64 t_begin = tq;
	(void)t_begin;
	if (lane < 36)
		L.llx[lane] = Z_LL_BASE[lane] | (u32)Z_LL_BITS[lane] << 24;
	if (lane < 53)
		L.mlx[lane] = Z_ML_BASE[lane] | (u32)Z_ML_BITS[lane] << 24;
	const u32 rec = blockIdx.x;
	if (rec >= nrec)
		return;
	/* a run (RUN) has no record and no frame header: its descriptor stands in for them.  The tables are device memory,
	 * so they are checked here.  Positions count from the start of the history in front of the run's output: a match
	 * may reach back that far and no further. */
	const ZRun R = RUN ? runs[rec] : ZRun{};
	if (RUN && (R.out_off > out_bytes || R.out_cap > out_bytes - R.out_off || R.hist > R.out_off ||
		    (u64)R.hist + R.out_cap > 0xFFFE0000ull || R.first > nblk || R.count > nblk - R.first || R.carry > 1 ||
		    stream_bytes > 0xFFFFFFF0ull)) {
		if (lane == 0) {
			out_len[rec] = 0;
			status[rec] = ST_BAD_RECORD;
		}
		return;
	}
	/* (carry_by_rec: the slot is the run's own copy in the scratch of gpumt_zstd_decompress_blocks_par, zstd_dec_par.h) */
	ZCarry *cy = RUN ? (ZCarry *)(carry_base + (size_t)(carry_by_rec ? rec : R.carry) * sizeof(ZCarry)) : nullptr;
	const u32 run_hist = R.hist, run_count = R.count, run_first = R.first, run_flags = R.flags;
	if (!RUN && wv_readfirst(status[rec]) != want_status)
		return; /* rejected by the probe kernel, or not this variant's record */
	if (!RUN && lane == 0)
		chk_valid[rec] = 0;
	const u64 roff = RUN ? 0 : rec_off[rec];
	const u32 rlen = RUN ? 12u : wv_readfirst(rec_len[rec]);
	const u8 *r = stream + roff;
	u8 *out = out_base + (RUN ? R.out_off - R.hist : out_off[rec]);
	const u32 cap = RUN ? R.hist + R.out_cap : wv_readfirst(out_len[rec]);
	u8 *lit_scratch = litbuf + (u64)rec * (RUN ? Z_RUN_LITSLOT : Z_LITSLOT);
	const u8 *mem_lo = stream, *mem_hi = stream + stream_bytes + 256; /* readable range */
	u32 stc = ST_OK;

	/* ---- record + frame header (RFC 8878 3.1.1) ---- */
	if (!RUN && (rlen < 12 + 6 || uld32(r) != ZMT_SKIP_MAGIC || uld32(r + 4) != 4 || uld32(r + 8) != rlen - 12)) {
		if (lane == 0)
			status[rec] = ST_BAD_RECORD;
		return;
	}
	const u8 *f = RUN ? stream : r + 12; /* (RUN: block positions are offsets into the stream, set block by block) */
	u32 flen = rlen - 12;
	if (!RUN && uld32(f) != ZMT_ZSTD_MAGIC) {
		if (lane == 0)
			status[rec] = ST_BAD_FRAME;
		return;
	}
	const u32 fhd = RUN ? 0u : uld8(f + 4);
	const u32 fcs = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3, has_chk = (fhd >> 2) & 1;
	u32 hp = 5;
	u64 window = 0, content = ~0ull;
	if (!RUN) {
		const u32 did_len = did == 3 ? 4 : did, fcs_len = fcs == 0 ? single : (1u << fcs);
		if ((fhd & 8) || flen < 5 + (1 - single) + did_len + fcs_len) {
			if (lane == 0)
				status[rec] = ST_BAD_FRAME;
			return;
		}
		if (did) {
			u32 id = 0;
			for (u32 i = 0; i < did_len; i++)
				id |= uld8(f + hp + (1 - single) + i);
			if (id) {
				if (lane == 0)
					status[rec] = ST_UNSUPPORTED;
				return;
			}
		}
		if (!single) {
			const u32 wd = uld8(f + hp++);
			const u64 base = 1ull << (10 + (wd >> 3));
			window = base + (base >> 3) * (wd & 7);
		}
		hp += did_len;
		if (fcs == 0 && single)
			content = uld8(f + hp);
		else if (fcs == 1)
			content = uld16(f + hp) + 256;
		else if (fcs == 2)
			content = uld32(f + hp);
		else if (fcs == 3)
			content = (u64)uld32(f + hp) | (u64)uld32(f + hp + 4) << 32;
		hp += fcs_len;
		if (single)
			window = content;
	}
	if (content != ~0ull && content != cap) {
		if (lane == 0)
			status[rec] = ST_SIZE_MISMATCH;
		return;
	}
	u32 block_max = window < Z_BLOCK_MAX ? (u32)window : Z_BLOCK_MAX;

	u32 rep0 = 1, rep1 = 4, rep2 = 8;
	bool huf_ok = false;
	int huf_log = 0;
	u32 pre_left = 0, pre_lit = 0; /* blocks ahead whose literals are already decoded / where they start */
	u32 sq_left = 0, sq_pos = 0; /* blocks (this one first) whose sequences are decoded / where they start */
	bool unit_head = false;
	u32 unit_n = 0; /* blocks behind a unit head whose sequence sections are listed in L.w */
	u64 *seq_scratch = (u64 *)(lit_scratch + Z_BLOCK_MAX + 256u);
	bool my_tab_ok = false; /* lanes 0..2: state of the LL / OF / ML table this lane builds */
	bool my_tab_pre = false; /* ... and whether it currently holds the predefined distribution */
	int my_tab_log = 0;
	u32 opos = run_hist, ip = hp;
	/* sequences decoded ahead by zmt_zstd_seq_kernel (zstd_dec_seq.hip): hdr[i] != 0 says block i's are at seq[hdr[i] - 1] */
	const bool pre_on = !RUN && seqbuf != nullptr && zs_eligible(seqcap, out_off[rec], cap);
	const u32 *pre_hdr = pre_on ? (const u32 *)zs_region(seqbuf, out_off[rec]) : nullptr;
	const u64 *pre_seq = pre_on ? zs_region(seqbuf, out_off[rec]) + zs_nhdr(cap) / 2 : nullptr;
	const u32 pre_nhdr = pre_on ? zs_nhdr(cap) : 0;
	u32 bi = 0; /* index of the block, counting every block of the frame */
	/* PRE: this block's mark and index in the table; the block that last defined the Huffman / LL / OF / ML table */
	u32 pmark = 0, pabs = 0, pd_huf = ZPRE_NONE, pd_ll = ZPRE_NONE, pd_of = ZPRE_NONE, pd_ml = ZPRE_NONE;
	bool pre_take = false;
	if constexpr (RUN) {
		/* ---- what the frame's earlier runs left: repeat offsets, the Huffman table, the three FSE tables ---- */
		if (!(run_flags & ZR_FIRST)) {
			if (cy->corrupt)
				stc = ZBAD(); /* an earlier run of this frame failed */
			rep0 = cy->rep[0];
			rep1 = cy->rep[1];
			rep2 = cy->rep[2];
			huf_ok = cy->huf_ok != 0 && cy->huf_log <= (u32)LDS::hcap;
			huf_log = huf_ok ? (int)cy->huf_log : 0;
			if (lane < 3) {
				my_tab_ok = cy->tab_ok[lane] != 0 &&
					    cy->tab_log[lane] <= (u32)(lane == 0 ? LDS::llcap : lane == 1 ? LDS::ofcap : LDS::mlcap);
				my_tab_log = my_tab_ok ? (int)cy->tab_log[lane] : 0;
				my_tab_pre = cy->tab_pre[lane] != 0;
			}
			for (u32 i = (u32)lane; i < (1u << LDS::hcap); i += 64)
				L.huf[i] = cy->huf[i];
			for (u32 i = (u32)lane; i < (1u << LDS::llcap); i += 64) {
				L.ll[i] = cy->ll[i];
				L.ml[i] = cy->ml[i];
			}
			for (u32 i = (u32)lane; i < (1u << LDS::ofcap); i += 64)
				L.of[i] = cy->of[i];
			wv_sync();
		}
	}

	for (; !RUN || (bi < run_count && stc == ST_OK);) {
		if constexpr (RUN) {
			const ZBlock B = blocks[run_first + bi];
			if (B.src_off > stream_bytes || B.src_len > stream_bytes - B.src_off || B.block_max > Z_BLOCK_MAX) {
				stc = ST_BAD_RECORD;
				break;
			}
			ip = (u32)B.src_off;
			flen = ip + B.src_len;
			block_max = B.block_max;
			if constexpr (PRE) {
				pabs = run_first + bi;
				pmark = wv_readfirst(pre_mark[pabs]);
			}
		}
		if (flen - ip < 3) {
			stc = ZBAD();
			break;
		}
		const u32 bh = uld8(f + ip) | uld8(f + ip + 1) << 8 | uld8(f + ip + 2) << 16;
		const u32 last = bh & 1, btype = (bh >> 1) & 3, bsize = bh >> 3;
		ip += 3;
		const u8 *src = f + ip;
		if (btype == 3 || bsize > block_max || (btype != 1 && flen - ip < bsize) ||
		    (btype == 1 && flen - ip < 1)) {
			stc = ZBAD();
			break;
		}
		if (btype == 0) {
			if (cap - opos < bsize) {
				stc = ST_SIZE_MISMATCH;
				break;
			}
			wave_copy(out + opos, src, bsize, lane);
			opos += bsize;
			ip += bsize;
		} else if (btype == 1) {
			if (cap - opos < bsize) {
				stc = ST_SIZE_MISMATCH;
				break;
			}
			const u8 v = (u8)uld8(src);
			for (u32 i = (u32)lane; i < bsize; i += 64)
				out[opos + i] = v;
			opos += bsize;
			ip += 1;
		} else {
			/* ================= compressed block ================= */
			ZP(6);
			const u32 bstart = opos;
			if (bsize < 2) {
				stc = ZBAD();
				break;
			}
			/* ---- literals section header + tree description, from LDS ---- */
			wv_sync();
			stage_load(L.stage, src, 0, 256, 0, mem_lo, mem_hi, lane);
			wv_sync();
			if (lane == 0) {
				const u8 *d = L.stage;
				const u32 ltype = d[0] & 3, sf = (d[0] >> 2) & 3;
				u32 regen = 0, csz = 0, hl = 0, streams = 1, err = 0, tree = 0;
				if (ltype < 2) {
					if (sf == 0 || sf == 2) {
						regen = d[0] >> 3;
						hl = 1;
					} else if (sf == 1) {
						regen = (d[0] | d[1] << 8) >> 4;
						hl = 2;
					} else {
						regen = (d[0] | d[1] << 8 | d[2] << 16) >> 4;
						hl = 3;
					}
					csz = ltype == 0 ? regen : 1;
				} else {
					const u64 v = (u64)ld32u(d) | (u64)d[4] << 32;
					if (sf < 2) {
						regen = (u32)(v >> 4) & 1023;
						csz = (u32)(v >> 14) & 1023;
						streams = sf == 0 ? 1 : 4;
						hl = 3;
					} else if (sf == 2) {
						regen = (u32)(v >> 4) & 16383;
						csz = (u32)(v >> 18) & 16383;
						streams = 4;
						hl = 4;
					} else {
						regen = (u32)(v >> 4) & 262143;
						csz = (u32)(v >> 22) & 262143;
						streams = 4;
						hl = 5;
					}
					if (regen == 0)
						err = 1;
				}
				if (regen > block_max || hl + csz > bsize)
					err = 1;
				if (!err && ltype == 2) {
					/* tree description: at most 1 + 128 bytes, inside the staged 256 */
					u32 avail = csz < 256 - hl ? csz : 256 - hl;
					int nw = 0, lg = 0;
					const int used = huf_read_weights(d + hl, avail, L.w, &nw, &lg, (u32 *)L.sq[0],
									  L.norm[0], L.next[0]);
					if (used < 0) {
						err = 1;
					} else {
						tree = (u32)used;
						L.misc[ZM_G] = (u32)nw;
						L.misc[ZM_H] = (u32)lg;
					}
				}
				L.misc[ZM_ERR] = err;
				L.misc[ZM_A] = ltype;
				L.misc[ZM_B] = regen;
				L.misc[ZM_C] = csz;
				L.misc[ZM_D] = hl;
				L.misc[ZM_E] = streams;
				L.misc[ZM_F] = tree;
			}
			wv_sync();
			if (L.misc[ZM_ERR]) {
				stc = ZBAD();
				break;
			}
			const u32 ltype = L.misc[ZM_A], regen = L.misc[ZM_B], lcsz = L.misc[ZM_C], lhl = L.misc[ZM_D];
			const u32 nstreams = L.misc[ZM_E], tree = L.misc[ZM_F];
			const u8 *lit = lit_scratch;
			if (ltype == 0) {
				lit = src + lhl;
				/* Raw literals (a unit whose literals did not compress): the blocks that follow the
				 * same way still share the predefined sequence tables; list them for the unit-wide
				 * sequence decode below (same records as the Huffman look-ahead writes) */
				if (!RUN && sq_left == 0 && !last) {
					u32 *pre = (u32 *)L.w;
					wv_sync();
					if (lane == 0) {
						u32 n = 0, q = ip + bsize;
						while (n < 15) {
							if (flen - q < 8)
								break;
							const u8 *h = f + q;
							const u32 bh2 = (u32)h[0] | (u32)h[1] << 8 | (u32)h[2] << 16;
							const u32 bs2 = bh2 >> 3;
							if (((bh2 >> 1) & 3) != 2 || bs2 > block_max || bs2 < 5 || flen - (q + 3) < bs2)
								break;
							const u32 b0 = h[3], sf2 = (b0 >> 2) & 3;
							if ((b0 & 3) != 0)
								break;
							u32 rg, hl2;
							if (sf2 == 1) {
								rg = (b0 | (u32)h[4] << 8) >> 4;
								hl2 = 2;
							} else if (sf2 == 3) {
								rg = (b0 | (u32)h[4] << 8 | (u32)h[5] << 16) >> 4;
								hl2 = 3;
							} else {
								rg = b0 >> 3;
								hl2 = 1;
							}
							if (rg > block_max || hl2 + rg > bs2)
								break;
							pre[4 * n] = q + 3 + hl2;
							pre[4 * n + 1] = rg;
							pre[4 * n + 3] = q + 3 + bs2;
							n++;
							q += 3 + bs2;
							if (bh2 & 1)
								break;
						}
						L.misc[ZM_A] = n;
					}
					wv_sync();
					unit_n = L.misc[ZM_A];
					unit_head = unit_n != 0;
				}
			} else if (ltype == 1) {
				const u8 v = (u8)uld8(src + lhl);
				for (u32 i = (u32)lane * 8; i < regen + 8; i += 512)
					st64g(lit_scratch + i, 0x0101010101010101ull * v);
			} else {
				if (ltype == 2) {
					const int nw = (int)L.misc[ZM_G];
					huf_log = (int)L.misc[ZM_H];
					if (huf_log > LDS::hcap) {
						stc = ST_NEEDS_GENERAL;
						break;
					}
					for (u32 i = (u32)lane; i < (1u << LDS::hcap); i += 64)
						L.huf[i] = 0;
					wv_sync();
					huf_fill(L.huf, L.w, nw, huf_log, lane);
					huf_ok = true;
					wv_sync();
				} else if (!huf_ok) {
					stc = ZBAD();
					break;
				}
				bool lit_done = false;
				if (ltype == 3 && pre_left) {
					/* decoded together with the block that carried the tree (below) */
					lit = lit_scratch + pre_lit;
					pre_lit += regen;
					pre_left--;
					lit_done = true;
				} else {
					pre_left = 0;
				}
				if constexpr (PRE) {
					if ((pmark & ZPRE_LIT) &&
					    (ltype == 2 || (pd_huf != ZPRE_NONE && wv_readfirst(pre_def[4 * (size_t)pabs]) == pd_huf))) {
						lit = pre_slots + (size_t)pabs * Z_PRE_STRIDE;
						lit_done = true;
					}
					if (ltype == 2)
						pd_huf = pabs;
				}
				/* ---- blocks that follow with `treeless` literals: all their streams at once ----
				 * The device encoder writes one tree per 128 KiB unit and up to 15 more blocks that
				 * reuse it; four lanes per block decode up to 64 streams side by side instead of 4.
				 * Anything odd in a block ahead just ends the look-ahead there: the block is then
				 * decoded (and judged) when its turn comes. */
				if (!RUN && ltype == 2 && nstreams == 4 && !last && lcsz >= tree + 10u) {
					u32 *pre = (u32 *)L.w; /* the weights are in the table now */
					wv_sync();
					if (lane == 0) {
						u32 n = 0, cum = regen, q = ip + bsize;
						while (n < 15) {
							if (flen - q < 8)
								break;
							const u8 *h = f + q;
							const u32 bh2 = (u32)h[0] | (u32)h[1] << 8 | (u32)h[2] << 16;
							const u32 bs2 = bh2 >> 3;
							if (((bh2 >> 1) & 3) != 2 || bs2 > block_max || bs2 < 5 || flen - (q + 3) < bs2)
								break;
							const u64 v = (u64)h[3] | (u64)h[4] << 8 | (u64)h[5] << 16 | (u64)h[6] << 24 | (u64)h[7] << 32;
							const u32 sf2 = (u32)(v >> 2) & 3;
							if ((v & 3) != 3 || sf2 == 0)
								break;
							u32 rg, cs, hl2;
							if (sf2 == 1) {
								rg = (u32)(v >> 4) & 1023;
								cs = (u32)(v >> 14) & 1023;
								hl2 = 3;
							} else if (sf2 == 2) {
								rg = (u32)(v >> 4) & 16383;
								cs = (u32)(v >> 18) & 16383;
								hl2 = 4;
							} else {
								rg = (u32)(v >> 4) & 262143;
								cs = (u32)(v >> 22) & 262143;
								hl2 = 5;
							}
							if (rg == 0 || rg > block_max || hl2 + cs > bs2 || cs < 10 || cum + rg > Z_BLOCK_MAX)
								break;
							pre[4 * n] = q + 3 + hl2; /* jump table, as an offset into the frame */
							pre[4 * n + 1] = cs;
							pre[4 * n + 2] = rg;
							pre[4 * n + 3] = q + 3 + bs2; /* end of the block */
							cum += rg;
							n++;
							q += 3 + bs2;
							if (bh2 & 1)
								break;
						}
						L.misc[ZM_A] = n;
					}
					wv_sync();
					u32 npre = L.misc[ZM_A];
					if (npre) {
						const u32 g = (u32)lane >> 2, sl = (u32)lane & 3;
						bool dec = g <= npre, bad = false;
						u32 jt = (u32)(src - f) + lhl + tree, cs = lcsz - tree, rg = regen, base = 0;
						if (g && dec) {
							jt = pre[4 * (g - 1)];
							cs = pre[4 * (g - 1) + 1];
							rg = pre[4 * (g - 1) + 2];
						}
						base = wv_scan_incl(sl == 0 && dec ? rg : 0u) - rg; /* literals of the blocks before mine */
						u32 s_off = 0, s_len = 0, s_n = 0, s_dst = 0;
						int ipos = 0;
						if (dec) {
							const u8 *jp = f + jt;
							const u32 j1 = (u32)jp[0] | (u32)jp[1] << 8, j2 = (u32)jp[2] | (u32)jp[3] << 8,
								  j3 = (u32)jp[4] | (u32)jp[5] << 8;
							const u32 tot = cs - 6, q4 = (rg + 3) / 4;
							if (j1 + j2 + j3 >= tot || 3 * q4 > rg) {
								bad = true;
							} else {
								s_off = jt + 6 + (sl > 0 ? j1 : 0) + (sl > 1 ? j2 : 0) + (sl > 2 ? j3 : 0);
								s_len = sl == 0 ? j1 : sl == 1 ? j2 : sl == 2 ? j3 : tot - j1 - j2 - j3;
								s_n = sl < 3 ? q4 : rg - 3 * q4;
								s_dst = base + sl * q4;
								const u32 lastb = s_len ? f[s_off + s_len - 1] : 0;
								if (s_len == 0 || lastb == 0)
									bad = true;
								else
									ipos = 8 * (int)(s_len - 1) + hb32(lastb);
							}
						}
						/* every lane keeps a 40-byte window of its own stream in LDS (over the
						 * header stage and the sequence batch, both idle here): 24 symbols a round
						 * (the sixth group of four starts at most 5 x 44 bits = 28 bytes down and
						 * reads 8 bytes from there) */
						u8 *win = L.below + 40u * (u32)lane;
						const int lg = huf_log;
						const u32 hm = (1u << lg) - 1;
						u32 done = 0;
						while (wv_any(dec && !bad && done < s_n)) {
							if (dec && !bad && done < s_n) {
								const int whi = (ipos + 7) >> 3, iwlo = whi - 40;
								const u8 *p = f + s_off + iwlo;
								u64 w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0;
								if (iwlo >= 0) {
									w0 = ld64u(p);
									w1 = ld64u(p + 8);
									w2 = ld64u(p + 16);
									w3 = ld64u(p + 24);
									w4 = ld64u(p + 32);
								} else {
									for (int k = 0; k < 8; k++) {
										if (iwlo + k >= 0)
											w0 |= (u64)p[k] << (8 * k);
										if (iwlo + 8 + k >= 0)
											w1 |= (u64)p[8 + k] << (8 * k);
										if (iwlo + 16 + k >= 0)
											w2 |= (u64)p[16 + k] << (8 * k);
										if (iwlo + 24 + k >= 0)
											w3 |= (u64)p[24 + k] << (8 * k);
										if (iwlo + 32 + k >= 0)
											w4 |= (u64)p[32 + k] << (8 * k);
									}
								}
								*(u64 *)win = w0;
								*(u64 *)(win + 8) = w1;
								*(u64 *)(win + 16) = w2;
								*(u64 *)(win + 24) = w3;
								*(u64 *)(win + 32) = w4;
								const u32 todo = s_n - done < 24 ? s_n - done : 24;
								u8 *dst = lit_scratch + s_dst + done;
								u32 i = 0;
								for (; i + 8 <= todo && ipos >= 0; i += 8) {
									u64 acc = 0;
									ZMT_UNROLL
									for (int hlf = 0; hlf < 2; hlf++) {
										const int tb = (ipos - 1) >> 3;
										const u64 word = ld64u(win + (tb - 7 - iwlo));
										int cb = ipos - 8 * (tb - 7);
										ZMT_UNROLL
										for (int k = 0; k < 4; k++) {
											const u32 e = L.huf[(u32)(word >> (cb - lg)) & hm];
											cb -= (int)(e >> 8);
											acc |= (u64)(e & 255) << (8 * (4 * hlf + k));
										}
										ipos = cb + 8 * (tb - 7);
									}
									st64g(dst + i, acc);
								}
								{
									u64 c = 0;
									int cb = 0;
									for (; i < todo && ipos >= 0; i++) {
										if (cb < lg) {
											const int tb = (ipos - 1) >> 3;
											c = ld64u(win + (tb - 7 - iwlo));
											cb = ipos - 8 * (tb - 7);
										}
										const u32 e = L.huf[(u32)(c >> (cb - lg)) & hm];
										const int nb = (int)(e >> 8);
										cb -= nb;
										ipos -= nb;
										dst[i] = (u8)e;
									}
								}
								if (ipos < 0)
									bad = true;
								done += todo;
								if (!bad && done == s_n && ipos != 0)
									bad = true;
							}
						}
						const u64 bm = wv_ballot(dec && bad);
						if (bm) {
							const u32 gb = (u32)(wv_ffs(bm) - 1) >> 2;
							if (gb == 0) {
								stc = ZBAD();
								break;
							}
							npre = gb - 1; /* the blocks from there on are decoded in their turn */
						}
						pre_left = npre;
						pre_lit = regen;
						lit_done = true;
						unit_head = npre != 0;
						unit_n = npre;
						wv_sync();
						wave_mem_fence();
					}
				}
				if (!lit_done) {
				ZP(0);
				/* ---- Huffman streams: lane s < nstreams decodes stream s ---- */
				const u32 body = lhl + tree; /* offset of jump table / single stream in src */
				if (lcsz < tree + (nstreams == 4 ? 10u : 1u)) {
					stc = ZBAD();
					break;
				}
				u32 s_off = body, s_len = lcsz - tree, s_n = regen, s_dst = 0;
				bool bad = false;
				if (nstreams == 4) {
					const u32 j1 = uld16(src + body), j2 = uld16(src + body + 2), j3 = uld16(src + body + 4);
					const u32 tot = lcsz - tree - 6, q = (regen + 3) / 4;
					if (j1 + j2 + j3 >= tot || 3 * q > regen) {
						stc = ZBAD();
						break;
					}
					const u32 sl = lane & 3;
					s_off = body + 6 + (sl > 0 ? j1 : 0) + (sl > 1 ? j2 : 0) + (sl > 2 ? j3 : 0);
					s_len = sl == 0 ? j1 : sl == 1 ? j2 : sl == 2 ? j3 : tot - j1 - j2 - j3;
					s_n = sl < 3 ? q : regen - 3 * q;
					s_dst = sl * q;
				}
				const bool dec = (u32)lane < nstreams;
				long pos = 0; /* unread bits of my stream */
				if (dec) {
					const u32 lastb = s_len ? src[s_off + s_len - 1] : 0;
					if (s_len == 0 || lastb == 0)
						bad = true;
					else
						pos = 8 * (long)(s_len - 1) + hb32(lastb);
				}
				if (wv_any(dec && bad)) {
					stc = ZBAD();
					break;
				}
				u32 done = 0;
				while (wv_any(dec && done < s_n && !bad)) {
					/* cooperative refill: 16 lanes per stream, 256-byte window ending at the
					 * byte that holds the next unread bit; bytes below the stream read 0 */
					wv_sync();
					{
						const int sg = lane >> 4;
						const u32 g_off = wv_shfl(s_off, sg);
						const u32 g_poslo = wv_shfl((u32)pos, sg);
						const u32 g_poshi = wv_shfl((u32)((u64)pos >> 32), sg);
						const long g_pos = (long)((u64)g_poshi << 32 | g_poslo);
						const long whi = (g_pos + 7) >> 3;
						if ((u32)sg < nstreams) {
							const u32 o = 16u * ((u32)lane & 15);
							const long rel = whi - 256 + (long)o;
							const u8 *p = src + g_off + rel;
							u64 a = 0, b = 0;
							if (rel >= 0 && p + 16 <= mem_hi) {
								a = ld64u(p);
								b = ld64u(p + 8);
							} else {
								for (int k = 0; k < 8; k++) {
									if (rel + k >= 0 && p + k < mem_hi)
										a |= (u64)p[k] << (8 * k);
									if (rel + 8 + k >= 0 && p + 8 + k < mem_hi)
										b |= (u64)p[8 + k] << (8 * k);
								}
							}
							u8 *w = L.stage + 256u * (u32)sg + o;
							*(u64 *)w = a;
							*(u64 *)(w + 8) = b;
						}
					}
					wv_sync();
					if (dec && !bad && done < s_n) {
						const u8 *win = L.stage + 256u * (u32)lane; /* byte (whi-256+i) of my stream */
						const long wlo = ((pos + 7) >> 3) - 256;
						const u32 todo = s_n - done < 128 ? s_n - done : 128;
						u8 *dst = lit_scratch + s_dst + done;
						const int lg = huf_log;
						const u32 hm = (1u << lg) - 1;
						int ipos = (int)pos; /* a stream holds < 2^21 bits */
						const int iwlo = (int)wlo;
						u32 i = 0;
						/* eight symbols per store; the container is refilled before every four
						 * (>= 57 fresh bits cover 4 x 11), so the symbol steps carry no branch */
						for (; i + 8 <= todo && ipos >= 0; i += 8) {
							u64 acc = 0;
							ZMT_UNROLL
							for (int hlf = 0; hlf < 2; hlf++) {
								const int tb = (ipos - 1) >> 3;
								const u64 word = ld64u(win + (tb - 7 - iwlo));
								int cb = ipos - 8 * (tb - 7);
								ZMT_UNROLL
								for (int k = 0; k < 4; k++) {
									const u32 e = L.huf[(u32)(word >> (cb - lg)) & hm];
									cb -= (int)(e >> 8);
									acc |= (u64)(e & 255) << (8 * (4 * hlf + k));
								}
								ipos = cb + 8 * (tb - 7);
							}
							st64g(dst + i, acc);
						}
						/* tail: fewer than eight symbols left in this round */
						{
							u64 c = 0;
							int cb = 0;
							for (; i < todo && ipos >= 0; i++) {
								if (cb < lg) {
									const int tb = (ipos - 1) >> 3;
									c = ld64u(win + (tb - 7 - iwlo));
									cb = ipos - 8 * (tb - 7);
								}
								const u32 e = L.huf[(u32)(c >> (cb - lg)) & hm];
								const int nb = (int)(e >> 8);
								cb -= nb;
								ipos -= nb;
								dst[i] = (u8)e;
							}
						}
						if (ipos < 0)
							bad = true; /* ran past the first bit of the stream */
						pos = ipos;
						done += todo;
						if (!bad && done == s_n && pos != 0)
							bad = true;
					}
				}
				if (wv_any(dec && bad)) {
					stc = ZBAD();
					break;
				}
				wave_mem_fence(); /* literals are read back by other lanes below */
				} /* !lit_done */
			}

			ZP(1);
			/* ---- sequences section header + table descriptions, from LDS ---- */
			const u32 sq0 = lhl + lcsz; /* offset of the sequences section in src */
			if (sq0 >= bsize) {
				stc = ZBAD();
				break;
			}
			/* decoded ahead by the pre-pass: only Number_of_Sequences is read here; the tables of this block are then
			 * not built (the pre-pass marks a prefix of the frame's blocks and leaves the decoder a block that describes
			 * all three tables itself, zstd_dec_seq.hip) */
			const u32 pre_at = (bi < pre_nhdr) ? wv_readfirst(pre_hdr[bi]) : 0u;
			const u64 *pseq = nullptr;
			u32 nseq, sq_hdr;
			bool all_pre = false, all_fit = false;
			if (pre_at) {
				const u32 s4 = uld32(src + sq0);
				nseq = s4 & 255;
				if (nseq == 255)
					nseq = ((s4 >> 8) & 0xFFFF) + 0x7F00;
				else if (nseq >= 128)
					nseq = ((nseq - 128) << 8) + ((s4 >> 8) & 255);
				sq_hdr = 0;
				pseq = pre_seq + (pre_at - 1);
				unit_head = false;
				sq_left = 0;
				if (lane < 3)
					my_tab_ok = false; /* what a repeat mode would refer to is not in this wave's LDS */
			} else {
			wv_sync();
			stage_load(L.stage, src, (long)sq0, 512, 0, mem_lo, mem_hi, lane);
			wv_sync();
			if (lane == 0) {
				const u8 *d = L.stage;
				const u32 avail = bsize - sq0 < 512 ? bsize - sq0 : 512;
				u32 p = 1, err = 0, nseq = d[0], modes = 0;
				if (nseq >= 128) {
					if (nseq == 255) {
						nseq = (d[1] | d[2] << 8) + 0x7F00;
						p = 3;
					} else {
						nseq = ((nseq - 128) << 8) + d[1];
						p = 2;
					}
				}
				if (p > avail)
					err = 1;
				if (!err && nseq) {
					if (p >= avail)
						err = 1;
					modes = d[p++];
					if (modes & 3)
						err = 1;
					for (int t = 0; t < 3 && !err; t++) {
						const int mode = (modes >> (6 - 2 * t)) & 3;
						const int max_sym = t == 0 ? 36 : t == 1 ? 32 : 53, max_log = t == 1 ? 8 : 9;
						L.misc[ZM_A + t] = 0xFFFFFFFFu; /* table stays as it is */
						if (mode == 0) {
							const short *def = t == 0 ? Z_LL_DEF : t == 1 ? Z_OF_DEF : Z_ML_DEF;
							const int n = t == 0 ? 36 : t == 1 ? 29 : 53;
							for (int i = 0; i < n; i++)
								L.norm[t][i] = def[i];
							L.misc[ZM_A + t] = (u32)n | (u32)(t == 1 ? 5 : 6) << 8 | 0x40000000u; /* predefined */
						} else if (mode == 1) {
							if (p >= avail || d[p] >= max_sym)
								err = 1;
							else
								L.misc[ZM_A + t] = 0x80000000u | d[p++]; /* RLE */
						} else if (mode == 2) {
							int nsym = 0, lg = 0;
							const int used = fse_read_ncount(d + p, avail - p, L.norm[t], max_sym, max_log, &nsym, &lg);
							if (used < 0) {
								err = 1;
							} else {
								p += (u32)used;
								L.misc[ZM_A + t] = (u32)nsym | (u32)lg << 8;
							}
						}
					}
				}
				L.misc[ZM_ERR] = err;
				L.misc[ZM_D] = nseq;
				L.misc[ZM_E] = p;
			}
			wv_sync();
			if (L.misc[ZM_ERR]) {
				stc = ZBAD();
				break;
			}
			nseq = L.misc[ZM_D];
			sq_hdr = L.misc[ZM_E];
			/* what the device encoder writes at the head of a unit: three predefined tables (the
			 * blocks behind it say "predefined" again), or three described ones (the blocks behind
			 * it say "repeat") */
			all_pre = nseq && (L.misc[ZM_A] & 0xC0000000u) == 0x40000000u &&
				  (L.misc[ZM_A + 1] & 0xC0000000u) == 0x40000000u &&
				  (L.misc[ZM_A + 2] & 0xC0000000u) == 0x40000000u;
			all_fit = nseq && L.misc[ZM_A] < 0x40000000u && L.misc[ZM_A + 1] < 0x40000000u &&
				  L.misc[ZM_A + 2] < 0x40000000u;
			if constexpr (PRE) {
				const bool r_ll = L.misc[ZM_A] == 0xFFFFFFFFu, r_of = L.misc[ZM_A + 1] == 0xFFFFFFFFu,
					   r_ml = L.misc[ZM_A + 2] == 0xFFFFFFFFu;
				const u32 *pd = pre_def + 4 * (size_t)pabs;
				pre_take = (pmark & ZPRE_SEQ) && nseq && nseq <= Z_PRE_SEQCAP(block_max) &&
					  (!r_ll || (pd_ll != ZPRE_NONE && wv_readfirst(pd[1]) == pd_ll)) &&
					  (!r_of || (pd_of != ZPRE_NONE && wv_readfirst(pd[2]) == pd_of)) &&
					  (!r_ml || (pd_ml != ZPRE_NONE && wv_readfirst(pd[3]) == pd_ml));
				if (nseq) {
					pd_ll = r_ll ? pd_ll : pabs;
					pd_of = r_of ? pd_of : pabs;
					pd_ml = r_ml ? pd_ml : pabs;
				}
			}
			}
			const u32 unit_modes = all_fit ? 0xFCu : 0u; /* Symbol_Compression_Modes of the unit's other blocks */
			u32 lpos = 0; /* literals consumed */
			if (nseq) {
				int ll_log = 0, of_log = 0, ml_log = 0;
				u32 bs_off = 0;
				long pos = 0;
				if (!pseq) {
				/* ---- build the three tables on lanes 0..2 ---- */
				bool terr = false, too_big = false;
				if (lane < 3) {
					const u32 spec = L.misc[ZM_A + lane];
					u32 *cells = lane == 0 ? L.ll : lane == 1 ? L.of : L.ml;
					if (spec == 0xFFFFFFFFu) {
						terr = !my_tab_ok; /* repeat mode needs a previous table */
					} else if (spec & 0x80000000u) {
						const u32 sy = spec & 255; /* RLE: one cell, no state bits */
						cells[0] = sy | (lane == 1 ? sy : (lane == 0 ? L.llx[sy] : L.mlx[sy]) >> 24) << 10;
						my_tab_log = 0;
						my_tab_ok = true;
						my_tab_pre = false;
					} else if ((spec & 0x40000000u) && my_tab_pre && my_tab_ok) {
						/* predefined table still in place from an earlier block: nothing to build */
					} else {
						const int lg = (int)((spec >> 8) & 255);
						if (lg > (lane == 0 ? LDS::llcap : lane == 1 ? LDS::ofcap : LDS::mlcap)) {
							too_big = true;
						} else {
						terr = fse_build(cells, L.norm[lane], (int)(spec & 255), lg, L.next[lane],
								 lane == 0 ? L.llx : lane == 2 ? L.mlx : (const u32 *)nullptr, lane) != 0;
						my_tab_log = lg;
						my_tab_ok = !terr;
						my_tab_pre = (spec & 0x40000000u) != 0;
						}
					}
				}
				wv_sync();
				if (wv_any(too_big)) {
					stc = ST_NEEDS_GENERAL;
					break;
				}
				if (wv_any(terr)) {
					stc = ZBAD();
					break;
				}
				ll_log = (int)wv_readlane((u32)my_tab_log, 0);
				of_log = (int)wv_readlane((u32)my_tab_log, 1);
				ml_log = (int)wv_readlane((u32)my_tab_log, 2);
				ZP(2);
				/* ---- FSE bitstream: src[sq0 + sq_hdr, bsize) read backwards ---- */
				bs_off = sq0 + sq_hdr;
				if (bs_off >= bsize) {
					stc = ZBAD();
					break;
				}
				const u32 bs_len = bsize - bs_off;
				const u32 lastb = uld8(src + bs_off + bs_len - 1);
				if (lastb == 0) {
					stc = ZBAD();
					break;
				}
				pos = 8 * (long)(bs_len - 1) + hb32(lastb); /* unread bits, wave-uniform */
				/* ---- unit: the sequences of this block and of the blocks looked at above ----
				 * Their bitstreams are independent and, with one set of tables for the unit, read
				 * through the same three tables: four lanes per block (LL / OF / ML state + one
				 * idle) decode up to 16 blocks side by side into the record's scratch, 8 bytes a
				 * sequence (ll | ml << 18 | offset value << 36); the blocks then only execute.
				 * As with the literals, anything odd ends the unit before that block. */
				if (!RUN && unit_head) {
					unit_head = false;
					sq_left = 0;
					if ((all_pre || all_fit) && unit_n) {
						const u32 *pre = (const u32 *)L.w;
						const u32 g = (u32)lane >> 2, sl = (u32)lane & 3;
						bool act = g <= unit_n, gbad = false;
						u32 g_off = (u32)(src - f) + bs_off, g_len = bs_len, g_n = nseq;
						if (g && act) {
							const u32 s0 = pre[4 * (g - 1)] + pre[4 * (g - 1) + 1], bend = pre[4 * (g - 1) + 3];
							g_n = 0;
							if (bend - s0 >= 4) {
								const u32 b0 = f[s0];
								u32 p = 1;
								g_n = b0;
								if (b0 == 255) {
									g_n = ((u32)f[s0 + 1] | (u32)f[s0 + 2] << 8) + 0x7F00u;
									p = 3;
								} else if (b0 >= 128) {
									g_n = ((b0 - 128) << 8) + f[s0 + 1];
									p = 2;
								}
								if (f[s0 + p] != unit_modes)
									g_n = 0; /* a table of its own */
								g_off = s0 + p + 1;
								if (g_off >= bend)
									g_n = 0;
								else
									g_len = bend - g_off;
							}
							if (g_n == 0)
								gbad = true;
						}
						int bp = 0; /* unread bits of my block's stream */
						if (act && !gbad) {
							const u32 lb = f[g_off + g_len - 1];
							if (lb == 0)
								gbad = true;
							else
								bp = 8 * (int)(g_len - 1) + hb32(lb);
							if (bp < ll_log + of_log + ml_log)
								gbad = true;
						}
						u32 ngrp = unit_n + 1;
						{
							const u64 bm = wv_ballot(act && gbad);
							if (bm)
								ngrp = (u32)(wv_ffs(bm) - 1) >> 2;
						}
						act = g < ngrp;
						const u32 incl = wv_scan_incl(sl == 0 && act ? g_n : 0u);
						{
							const u64 om = wv_ballot(act && incl > Z_SEQCAP);
							if (om)
								ngrp = (u32)(wv_ffs(om) - 1) >> 2;
						}
						act = g < ngrp;
						u64 *myseq = seq_scratch + (incl - g_n);
						if (ngrp >= 2) {
							const u32 *mytab = sl == 1 ? L.of : sl == 2 ? L.ml : L.ll;
							const u32 mylog = sl == 0 ? (u32)ll_log : sl == 1 ? (u32)of_log : sl == 2 ? (u32)ml_log : 0u;
							const u32 tmask = (1u << mylog) - 1;
							const u32 e_of = sl == 1 ? 0u : ~0u, e_ml = sl == 0 ? ~0u : 0u;
							const u32 s_ll = sl == 0 ? 0u : ~0u, s_ml = sl == 1 ? ~0u : 0u;
							u8 *gwin = L.below + 160u * g; /* 160-byte window per block, 40 per lane */
							u32 state = 0, done = 0;
							bool first = true;
							while (wv_any(act && done < g_n)) {
								const int whi = (bp + 7) >> 3, wlo = whi - 160;
								wv_sync();
								if (act && done < g_n) {
									const int rel = (int)g_off + wlo + 40 * (int)sl;
									u64 w[5] = {0, 0, 0, 0, 0};
									if (rel >= 0) {
										ZMT_UNROLL
										for (int j = 0; j < 5; j++)
											w[j] = ld64u(f + rel + 8 * j);
									} else {
										for (int j = 0; j < 5; j++)
											for (int k2 = 0; k2 < 8; k2++)
												if (rel + 8 * j + k2 >= 0)
													w[j] |= (u64)f[rel + 8 * j + k2] << (8 * k2);
									}
									ZMT_UNROLL
									for (int j = 0; j < 5; j++)
										*(u64 *)(gwin + 40u * sl + 8u * (u32)j) = w[j];
								}
								wv_sync();
								const u8 *winb = gwin - wlo - 15; /* winb[b + 15] = byte b of my stream */
								if (first) {
									first = false;
									const int tb = (bp - 1) >> 3;
									const u64 w1 = ld64u(winb + tb), w0 = ld64u(winb + tb + 8);
									const u32 skip = (u32)(8 * (tb + 1) - bp);
									state = xbits(w0, w1, skip + (sl == 0 ? 0u : sl == 1 ? (u32)ll_log : (u32)(ll_log + of_log)),
										      mylog);
									bp -= ll_log + of_log + ml_log;
								}
								for (;;) {
									/* eight sequences of every block; lane sl keeps 2 sl, 2 sl + 1 */
									u64 r0 = 0, r1 = 0;
									ZMT_UNROLL
									for (int i = 0; i < 8; i++) {
										const bool on = act && done + (u32)i < g_n;
										int tb = (bp - 1) >> 3;
										tb = tb < wlo + 15 ? wlo + 15 : tb; /* a stream gone bad stays inside its window */
										u64 w1, w0;
										lds_ld128(winb + tb, w1, w0);
										const u32 cell = mytab[state & tmask];
										const u32 skip = (u32)(8 * (tb + 1) - bp) & 127u;
										const u32 nb = done + (u32)i + 1 == g_n ? 0u : ZC_NB(cell), ab = ZC_AB(cell);
										const u32 pk = ab | nb << 8;
										const u32 p_ll = wv_quad(pk, 0), p_of = wv_quad(pk, 1), p_ml = wv_quad(pk, 2);
										const u32 a_ll = p_ll & 255, n_ll = p_ll >> 8, a_of = p_of & 255, n_of = p_of >> 8;
										const u32 a_ml = p_ml & 255, n_ml = p_ml >> 8;
										const u32 base3 = skip + a_of + a_ml + a_ll;
										const u32 eo = skip + (a_of & e_of) + (a_ml & e_ml);
										const u32 so = base3 + (n_ll & s_ll) + (n_ml & s_ml);
										const u32 extra = xbits(w0, w1, eo, ab);
										const u32 sbits = xbits(w0, w1, so, nb);
										const u32 sym = ZC_SYM(cell);
										const u32 val = sl == 0   ? (L.llx[sym < 36 ? sym : 0] & 0xFFFFFFu) + extra
												: sl == 2 ? (L.mlx[sym < 53 ? sym : 0] & 0xFFFFFFu) + extra
													  : (1u << (sym & 31)) + extra;
										if (on && sl == 1 && sym > 27)
											gbad = true; /* does not fit the packing: left to the block itself */
										const u32 v_ll = wv_quad(val, 0), v_of = wv_quad(val, 1), v_ml = wv_quad(val, 2);
										const u64 rcd = (u64)v_ll | (u64)v_ml << 18 | (u64)v_of << 36;
										if ((u32)(i >> 1) == sl) {
											if (i & 1)
												r1 = rcd;
											else
												r0 = rcd;
										}
										state = on ? ZC_BASE(cell) + sbits : state;
										bp -= on ? (int)(base3 - skip + n_ll + n_ml + n_of) : 0;
									}
									if (act && done + 2 * sl < g_n)
										st64g((u8 *)(myseq + done + 2 * sl), r0);
									if (act && done + 2 * sl + 1 < g_n)
										st64g((u8 *)(myseq + done + 2 * sl + 1), r1);
									if (act && done < g_n) {
										done = g_n - done < 8 ? g_n : done + 8;
										if (bp < 0 || (done == g_n && bp != 0))
											gbad = true;
										if (gbad)
											act = false;
									}
									const bool more = act && done < g_n;
									/* 8 x 76 more bits and the 16-byte read must stay inside the 160 bytes */
									if (!wv_any(more) || wv_any(more && 8 * whi - bp > 544))
										break;
								}
							}
							wave_mem_fence();
							{
								const u64 bm = wv_ballot(gbad && g < ngrp);
								if (bm) {
									const u32 gb = (u32)(wv_ffs(bm) - 1) >> 2;
									ngrp = gb < ngrp ? gb : ngrp;
								}
							}
							sq_left = ngrp;
							sq_pos = 0;
#ifdef ZMT_EMU
							if (getenv("ZMT_EMU_DEBUG") && lane == 0)
								fprintf(stderr, "zstd_dec: unit of %u blocks decoded side by side (%s tables)\n", ngrp,
									all_fit ? "described" : "predefined");
#endif
							wv_sync();
						}
					}
				}
				} /* !pseq */
				if constexpr (PRE) {
					if (pre_take)
						pseq = (const u64 *)(pre_slots + (size_t)pabs * Z_PRE_STRIDE + Z_PRE_LIT);
				}
				const bool from_scr = sq_left != 0 || pseq != nullptr;
				/* lanes 0 / 1 / 2 carry the LL / OF / ML state and decode their own code; the
				 * loop below is wave-uniform (one LDS round trip per sequence): every lane reads
				 * its state's cell and the same 128-bit window of the bitstream, the six field
				 * widths are exchanged through SGPRs, each lane cuts its two fields out */
				const u32 *mytab = lane == 1 ? L.of : lane == 2 ? L.ml : L.ll;
				u64 *myval = L.sq[lane < 3 ? lane : 0];
				/* where a lane's two fields start, as masks over the widths of the others: the
				 * stream order is OF extra, ML extra, LL extra, LL state, ML state, OF state */
				const u32 e_of = lane == 1 ? 0u : ~0u, e_ml = lane == 0 ? ~0u : 0u;
				const u32 s_ll = lane == 0 ? 0u : ~0u, s_ml = lane == 1 ? ~0u : 0u;
				u32 state = 0;
				for (u32 sbase = 0; sbase < nseq && stc == ST_OK; sbase += 64) {
					const u32 k = nseq - sbase < 64 ? nseq - sbase : 64;
					const bool act0 = (u32)lane < k;
					u32 ll = 0, ml = 0, ofv = 4;
					if (!from_scr) {
					/* window of the bitstream: 1 KiB ending at the byte of the next unread bit */
					const long whi = (pos + 7) >> 3, wlo = whi - (long)Z_STAGE;
					wv_sync();
					stage_load(L.stage, src + bs_off, wlo, Z_STAGE, -(long)(bs_off + 16), mem_lo, mem_hi, lane);
					wv_sync();
					const u8 *win = L.stage - wlo; /* win[b] = byte b of the bitstream */
					bool err = false;
					if (sbase == 0) {
						/* initial states: LL, OF, ML (RFC 8878 3.1.1.3.2.1.1) */
						if (pos < (long)(ll_log + of_log + ml_log)) {
							stc = ZBAD();
							break;
						}
						const long tb = (pos - 1) >> 3;
						const u64 w0 = ld64u(win + tb - 7), w1 = ld64u(win + tb - 15);
						const u32 skip = (u32)(8 * (tb + 1) - pos);
						state = xbits(w0, w1, skip + (lane == 0 ? 0u : lane == 1 ? (u32)ll_log : (u32)(ll_log + of_log)),
							      (u32)(lane < 3 ? my_tab_log : 0));
						pos -= ll_log + of_log + ml_log;
					}
					int bp = (int)pos; /* a sequences bitstream holds < 2^21 bits */
					const u8 *winb = win - 15;
					for (u32 i = 0; i < k; i++) {
						/* bp == 0 is legal here: the last sequence may need no bits at all; a
						 * negative bp is caught after the loop (the reads then come from the
						 * slack below the window).  Both LDS reads of the step are issued
						 * together: one round trip per sequence. */
						const int tb = (bp - 1) >> 3;
						/* only the three state lanes read the window: a misaligned 8-byte LDS read costs the CU's LDS
						 * pipe one cycle per ACTIVE lane (tools/ubench/lds_cost.hip) -- with all 64 lanes reading the
						 * same two addresses this loop was bound by that pipe, 128 cycles per sequence and wave */
						u64 w1 = 0, w0 = 0;
						if (lane < 3) {
							w1 = ld64u(winb + tb);
							w0 = ld64u(winb + tb + 8);
						}
						const u32 cell = mytab[state];
						const u32 skip = (u32)(8 * (tb + 1) - bp);
						const u32 nb = sbase + i + 1 == nseq ? 0u : ZC_NB(cell), ab = ZC_AB(cell);
						const u32 pk = ab | nb << 8;
						const u32 p_ll = wv_readlane(pk, 0), p_of = wv_readlane(pk, 1), p_ml = wv_readlane(pk, 2);
						const u32 a_ll = p_ll & 255, n_ll = p_ll >> 8, a_of = p_of & 255, n_of = p_of >> 8;
						const u32 a_ml = p_ml & 255, n_ml = p_ml >> 8;
						const u32 base3 = skip + a_of + a_ml + a_ll;
						const u32 eo = skip + (a_of & e_of) + (a_ml & e_ml);
						const u32 so = base3 + (n_ll & s_ll) + (n_ml & s_ml);
						const u32 extra = xbits(w0, w1, eo, ab);
						const u32 sbits = xbits(w0, w1, so, nb);
						if (lane < 3)
							myval[i] = (u64)extra | (u64)ZC_SYM(cell) << 32;
						state = lane < 3 ? ZC_BASE(cell) + sbits : 0;
						bp -= (int)(base3 - skip + n_ll + n_ml + n_of);
					}
					pos = bp;
					if (err || pos < 0 || (sbase + k == nseq && pos != 0)) {
						stc = ZBAD();
						break;
					}
					wv_sync();
					ZP(3);
					/* ---- execute the k sequences ---- */
					if (act0) {
						const u64 q_ll = L.sq[0][lane], q_of = L.sq[1][lane], q_ml = L.sq[2][lane];
						const u32 c_of = (u32)(q_of >> 32);
						ll = (L.llx[(u32)(q_ll >> 32)] & 0xFFFFFFu) + (u32)q_ll;
						ml = (L.mlx[(u32)(q_ml >> 32)] & 0xFFFFFFu) + (u32)q_ml;
						ofv = c_of > 31 ? 0u : (1u << c_of) + (u32)q_of;
					}
					} else if (act0) {
						const u64 v = (pseq ? pseq : seq_scratch + sq_pos)[sbase + (u32)lane];
						ll = (u32)v & 0x3FFFFu;
						ml = (u32)(v >> 18) & 0x3FFFFu;
						ofv = (u32)(v >> 36);
					}
					if (wv_any(act0 && ofv == 0)) {
						stc = ZBAD(); /* offset code > 31 */
						break;
					}
					/* repeat offsets (RFC 8878 3.1.1.5): runs of new offsets fold into the history in
					 * one step, only the sequences that use a repeat code are walked one by one */
					u32 off = ofv - 3;
					if (z_rep_fold(ofv, ll, act0, k, rep0, rep1, rep2, off, lane)) {
						stc = ZBAD();
						break;
					}
					const u32 len = ll + ml;
					const u32 incl = wv_scan_incl(len), lincl = wv_scan_incl(ll);
					const u32 tot = wv_readlane(incl, 63), ltot = wv_readlane(lincl, 63);
					/* 64 x (2 x 131074) cannot wrap 32 bits */
					if (ltot > regen - lpos || tot > cap - opos || opos + tot - bstart > block_max) {
						stc = ZBAD();
						break;
					}
					const u32 op = opos + incl - len, mpos = op + ll, lsrc = lpos + lincl - ll;
					if (wv_any(act0 && off > mpos)) {
						stc = ZBAD(); /* reaches before the start of the frame */
						break;
					}
					const u32 src_pos = mpos - off, eff = ml < off ? ml : off;
					const u64 longm = wv_ballot(act0 && (ll > Z_CAP || ml > Z_CAP));
					/* literals: independent of everything in this batch */
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
					wave_mem_fence();
					ZP(4);
					/* matches: watermark rounds.  W = everything below is written and visible */
					{
						bool fin = !act0;
						for (;;) {
							const u64 unf = wv_ballot(!fin);
							if (!unf)
								break;
							const int fst = wv_ffs(unf) - 1;
							const u32 W = wv_readlane(mpos, fst);
							if ((longm >> fst) & 1 && wv_readlane(ml, fst) > Z_CAP) {
								/* long match at the head of the queue: whole wave */
								wave_match(out + W, wv_readlane(off, fst), wv_readlane(ml, fst), lane);
								if (lane == fst)
									fin = true;
							} else {
								const bool ready = !fin && ml <= Z_CAP && src_pos + eff <= W;
								if (ready) {
									g_match(out + mpos, off, ml);
									fin = true;
								}
							}
							wave_mem_fence();
						}
					}
					ZP(5);
					opos += tot;
					lpos += ltot;
				}
				if (stc != ST_OK)
					break;
				if (sq_left) {
					sq_pos += nseq;
					sq_left--;
				}
			} else if (sq_hdr != bsize - sq0) {
				stc = ZBAD();
				break;
			}
			/* literals after the last sequence */
			{
				const u32 restl = regen - lpos;
				if (restl > cap - opos || opos + restl - bstart > block_max) {
					stc = ZBAD();
					break;
				}
				wave_copy(out + opos, lit + lpos, restl, lane);
				opos += restl;
			}
			wave_mem_fence();
			unit_head = false;
			ip += bsize;
		}
		bi++;
		if constexpr (RUN) {
			if (ip != flen) {
				stc = ZBAD(); /* the table entry is not the block its header describes */
				break;
			}
		} else if (last) {
			break;
		}
	}
	if constexpr (RUN) {
		/* ---- the run's verdict, and the state for the frame's next run ---- */
		wv_sync();
		if (!(run_flags & ZR_LAST)) {
			if (lane == 0) {
				cy->rep[0] = rep0;
				cy->rep[1] = rep1;
				cy->rep[2] = rep2;
				cy->huf_ok = huf_ok;
				cy->huf_log = (u32)huf_log;
				cy->corrupt = stc != ST_OK;
			}
			if (lane < 3) {
				cy->tab_ok[lane] = my_tab_ok;
				cy->tab_log[lane] = (u32)my_tab_log;
				cy->tab_pre[lane] = my_tab_pre;
			}
			for (u32 i = (u32)lane; i < (1u << LDS::hcap); i += 64)
				cy->huf[i] = L.huf[i];
			for (u32 i = (u32)lane; i < (1u << LDS::llcap); i += 64) {
				cy->ll[i] = L.ll[i];
				cy->ml[i] = L.ml[i];
			}
			for (u32 i = (u32)lane; i < (1u << LDS::ofcap); i += 64)
				cy->of[i] = L.of[i];
		}
		if (lane == 0) {
			out_len[rec] = opos - run_hist;
			status[rec] = stc;
		}
		return;
	}
	ZP(6);
#ifndef ZMT_EMU
	if (PROF && prof && lane == 0) {
		for (int i = 0; i < (PROF ? 7 : 1); i++)
			atomicAdd(prof + i, (unsigned long long)pc[i]);
		atomicAdd(prof + 8, (unsigned long long)(ZT() - t_begin));
		atomicAdd(prof + 9, 1ull);
	}
#endif
	/* a frame that states its content size must produce exactly that (= the caller's out_len); one
	 * that does not (streaming writers; never zstd-mt) was given a capacity and reports its size */
	if (stc == ST_OK && content != ~0ull && opos != cap)
		stc = ST_SIZE_MISMATCH;
	if (stc == ST_OK && content == ~0ull && lane == 0)
		out_len[rec] = opos;
	if (stc == ST_OK && has_chk) {
		/* Content_Checksum: low 32 bits of XXH64 of the content (RFC 8878 3.1.1); compared by
		 * zmt_xxh64_verify_kernel once the content is complete.  zstd-mt never writes one
		 * (one-shot ZSTD_compress, lib/zstd-mt_compress.c:285); the zstd CLI does. */
		if (flen - ip < 4) {
			stc = ST_BAD_FRAME;
		} else {
			if (lane == 0) {
				chk_expect[rec] = ld32u(f + ip);
				chk_valid[rec] = 1;
			}
			ip += 4;
		}
	}
	if (stc == ST_OK && ip != flen)
		stc = ST_TRAILING;
	if (lane == 0 && (stc != ST_OK || want_status != ST_OK))
		status[rec] = stc;
}

#ifdef ZMT_EMU
#define ZMT_WAVES4
#else
#ifndef ZD_WAVES
#define ZD_WAVES 4 /* 128 VGPRs: 16 waves per CU */
#endif
#define ZMT_WAVES4 __attribute__((amdgpu_waves_per_eu(ZD_WAVES, ZD_WAVES)))
#endif
/* records whose status is `want` (GPUMT_ST_OK after the probe, or ST_NEEDS_GENERAL after the small
 * variant) are decoded; their status becomes OK / an error / ST_NEEDS_GENERAL (small variant only) */
extern "C" __global__ void __launch_bounds__(64) ZMT_WAVES4
zmt_zstd_dec_small_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const u64 *__restrict__ rec_off,
			  const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base,
			  const u64 *__restrict__ out_off, u32 *__restrict__ out_len,
			  u8 *__restrict__ litbuf, u32 *__restrict__ status, u32 *__restrict__ chk_expect,
			  u32 *__restrict__ chk_valid, u8 *seqbuf, u64 seqcap)
{
	__shared__ __attribute__((aligned(16))) ZLdsSmall L;
	zstd_dec_body<false>(L, (u32)ST_OK, stream, stream_bytes, rec_off, rec_len, nrec, out_base, out_off, out_len,
			     litbuf, status, chk_expect, chk_valid, nullptr, seqbuf, seqcap);
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_dec_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const u64 *__restrict__ rec_off,
		    const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base,
		    const u64 *__restrict__ out_off, u32 *__restrict__ out_len,
		    u8 *__restrict__ litbuf, u32 *__restrict__ status, u32 *__restrict__ chk_expect,
		    u32 *__restrict__ chk_valid, u32 want, u8 *seqbuf, u64 seqcap)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	zstd_dec_body<false>(L, want, stream, stream_bytes, rec_off, rec_len, nrec, out_base, out_off, out_len, litbuf,
			     status, chk_expect, chk_valid, nullptr, seqbuf, seqcap);
}

#ifndef ZMT_EMU
/* same kernel with per-phase cycle counters (developer tool) */
extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_dec_kernel_prof(const u8 *__restrict__ stream, u64 stream_bytes, const u64 *__restrict__ rec_off,
			 const u32 *__restrict__ rec_len, u32 nrec, u8 *out_base,
			 const u64 *__restrict__ out_off, u32 *__restrict__ out_len,
			 u8 *__restrict__ litbuf, u32 *__restrict__ status, u32 *__restrict__ chk_expect,
			 u32 *__restrict__ chk_valid, u32 want, unsigned long long *prof, u8 *seqbuf, u64 seqcap)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	zstd_dec_body<true>(L, want, stream, stream_bytes, rec_off, rec_len, nrec, out_base, out_off, out_len, litbuf,
			    status, chk_expect, chk_valid, prof, seqbuf, seqcap);
}
#endif

/* One wave per run of blocks, full-size tables: status[r] = GPUMT_ST_OK / BAD_BLOCK / BAD_RECORD (a table entry that
 * leaves the stream or the output), run_len[r] = bytes decoded.  A match may read the run's `hist` bytes in front of its
 * output and no further; a treeless or Repeat_Mode block whose table neither this run nor the carry holds is BAD_BLOCK. */
extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_dec_run_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			const ZRun *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes, u8 *carry,
			u32 *__restrict__ run_len, u32 *__restrict__ status, u8 *__restrict__ litbuf)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	zstd_dec_body<false, ZLds, true>(L, 0u, stream, stream_bytes, nullptr, nullptr, nrun, out_base, nullptr, run_len, litbuf,
					 status, nullptr, nullptr, nullptr, nullptr, 0, blocks, nblk, runs, out_bytes, carry);
}

/* ------------------------------------------------------------------ the entropy pre-pass of a block table
 * gpumt_zstd_decompress_blocks_pre: a run is one chain on one wave only where the format makes it one -- repeat offsets and
 * matches that read earlier output.  A block's Huffman literals and its FSE sequence bitstream depend on nothing earlier
 * blocks produced, only on tables that some earlier block may have described.  Four launches on the caller's stream, none of
 * which waits on another wave (the stream orders them):
 *   classify  one lane per block: the block, literals-section and sequences-section headers -> ZPre
 *   resolve   one wave per run: for every block, the nearest earlier block of the run (in this call) that describes the
 *             Huffman / LL / OF / ML table it would use -> def
 *   entropy   one wave per Compressed_Block of the whole table: builds the block's tables in LDS from its own description
 *             or its definer's bytes, decodes the literals and the sequences (ll | ml << 18 | offset value << 36, the
 *             packing of zstd_dec_seq.hip; repeat codes stay codes) into the block's slots -> mark
 *   execute   zmt_zstd_dec_run_pre_kernel, one wave per run: zstd_dec_body<RUN, PRE>
 * A mark is set only when everything the serial walk checks on the way was clean, with the serial decoder's own code for
 * the tables and the same steps for the bitstreams; whatever is odd stays unmarked and is judged by the run kernel's code.
 * The tables are device memory and the input may be hostile: every read is inside [stream, stream + stream_bytes + 256),
 * every write inside the block's slots. */
extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_pre_classify_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			     ZPre *__restrict__ pre, u32 *__restrict__ def, u32 *__restrict__ mark)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nblk)
		return;
	ZPre P = {0, 0, 0, 0, 0, 0, 0, 0};
	const ZBlock B = blocks[i];
	if (B.src_off <= stream_bytes && B.src_len <= stream_bytes - B.src_off && B.block_max <= Z_BLOCK_MAX && B.src_len >= 5) {
		const u8 *h = stream + B.src_off;
		const u32 bh = (u32)h[0] | (u32)h[1] << 8 | (u32)h[2] << 16;
		const u32 bsize = bh >> 3;
		if (((bh >> 1) & 3) == 2 && bsize <= B.block_max && bsize == B.src_len - 3) {
			const u8 *d = h + 3;
#define ZPB(k) ((k) < bsize ? (u32)d[k] : 0u) /* (a header that leaves the block fails its size check below) */
			const u32 b0 = ZPB(0), ltype = b0 & 3, sf = (b0 >> 2) & 3;
			u32 regen = 0, csz = 0, hl = 0, streams = 1, err = 0;
			if (ltype < 2) {
				if (sf == 0 || sf == 2) {
					regen = b0 >> 3;
					hl = 1;
				} else if (sf == 1) {
					regen = (b0 | ZPB(1) << 8) >> 4;
					hl = 2;
				} else {
					regen = (b0 | ZPB(1) << 8 | ZPB(2) << 16) >> 4;
					hl = 3;
				}
				csz = ltype == 0 ? regen : 1;
			} else {
				const u64 v = (u64)(b0 | ZPB(1) << 8 | ZPB(2) << 16 | ZPB(3) << 24) | (u64)ZPB(4) << 32;
				if (sf < 2) {
					regen = (u32)(v >> 4) & 1023;
					csz = (u32)(v >> 14) & 1023;
					streams = sf == 0 ? 1 : 4;
					hl = 3;
				} else if (sf == 2) {
					regen = (u32)(v >> 4) & 16383;
					csz = (u32)(v >> 18) & 16383;
					streams = 4;
					hl = 4;
				} else {
					regen = (u32)(v >> 4) & 262143;
					csz = (u32)(v >> 22) & 262143;
					streams = 4;
					hl = 5;
				}
				if (regen == 0)
					err = 1;
			}
			if (regen > B.block_max || hl + csz >= bsize)
				err = 1; /* (== : no sequences section) */
			if (!err) {
				const u32 sq0 = hl + csz, avail = bsize - sq0 < 512 ? bsize - sq0 : 512;
				u32 p = 1, nseq = ZPB(sq0), modes = 0;
				if (nseq >= 128) {
					if (nseq == 255) {
						nseq = (ZPB(sq0 + 1) | ZPB(sq0 + 2) << 8) + 0x7F00;
						p = 3;
					} else {
						nseq = ((nseq - 128) << 8) + ZPB(sq0 + 1);
						p = 2;
					}
				}
				if (p > avail)
					err = 1;
				if (!err && nseq) {
					if (p >= avail)
						err = 1;
					modes = ZPB(sq0 + p);
					p++;
					if (modes & 3)
						err = 1;
				} else if (!err && p != bsize - sq0) {
					err = 1; /* no sequences: the section is its count alone */
				}
				if (!err) {
					P.ok = 1;
					P.lit = ltype | streams << 2 | hl << 8;
					P.regen = regen;
					P.lcsz = csz;
					P.sq0 = sq0;
					P.nseq = nseq;
					P.sqh = p | modes << 8;
					P.bsize = bsize;
				}
			}
#undef ZPB
		}
	}
	pre[i] = P;
	mark[i] = 0;
	for (int k = 0; k < 4; k++)
		def[4 * (size_t)i + k] = ZPRE_NONE;
}

/* lanes 0..3 = Huffman, LL, OF, ML: each walks the run's blocks in order and notes, per block, the last definer so far */
extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_pre_resolve_kernel(const ZRun *__restrict__ runs, u32 nrun, u32 nblk, const ZPre *__restrict__ pre,
			    u32 *__restrict__ def, u32 *__restrict__ run_last)
{
	const u32 r = blockIdx.x;
	const int lane = wv_lane();
	if (r >= nrun || lane >= 4)
		return;
	const ZRun R = runs[r];
	if (R.first > nblk || R.count > nblk - R.first)
		return;
	u32 last = ZPRE_NONE;
	for (u32 b = R.first; b < R.first + R.count; b++) {
		const ZPre P = pre[b];
		if (!P.ok)
			continue; /* raw, RLE: no tables; unparseable: the run ends there */
		if (lane == 0) {
			if ((P.lit & 3) == 2)
				last = b;
			if ((P.lit & 3) >= 2)
				def[4 * (size_t)b] = last;
		} else if (P.nseq) {
			if (((P.sqh >> (16 - 2 * lane)) & 3) != 3) /* modes << 8: LL at bits 14-15, OF 12-13, ML 10-11 */
				last = b;
			def[4 * (size_t)b + (u32)lane] = last;
		}
	}
	if (run_last) /* the run's last definer of each table (the carry kernel of zstd_dec_par.h) */
		run_last[4 * (size_t)r + (u32)lane] = last;
}

/* the sequences-section header of block `P` at body `src`: the descriptions of the tables in `want` (bit t) go to
 * L.norm[t] / L.misc[ZM_A + t] as in zstd_dec_body, L.misc[ZM_E] = where the bitstream starts.  Wave-uniform. */
template <typename LDS>
static __device__ bool zpre_seq_header(LDS &L, const u8 *src, const ZPre &P, u32 want, const u8 *mem_lo, const u8 *mem_hi,
				       int lane)
{
	wv_sync();
	stage_load(L.stage, src, (long)P.sq0, 512, 0, mem_lo, mem_hi, lane);
	wv_sync();
	if (lane == 0) {
		const u8 *d = L.stage;
		const u32 avail = P.bsize - P.sq0 < 512 ? P.bsize - P.sq0 : 512, modes = P.sqh >> 8;
		u32 p = P.sqh & 255, err = 0;
		for (int t = 0; t < 3 && !err; t++) {
			const int mode = (modes >> (6 - 2 * t)) & 3;
			const int max_sym = t == 0 ? 36 : t == 1 ? 32 : 53, max_log = t == 1 ? 8 : 9;
			u32 spec = 0xFFFFFFFFu;
			if (mode == 0) {
				if ((want >> t) & 1) {
					const short *df = t == 0 ? Z_LL_DEF : t == 1 ? Z_OF_DEF : Z_ML_DEF;
					const int n = t == 0 ? 36 : t == 1 ? 29 : 53;
					for (int i = 0; i < n; i++)
						L.norm[t][i] = df[i];
					spec = (u32)n | (u32)(t == 1 ? 5 : 6) << 8 | 0x40000000u;
				}
			} else if (mode == 1) {
				if (p >= avail || d[p] >= max_sym)
					err = 1;
				else
					spec = 0x80000000u | d[p++];
			} else if (mode == 2) {
				int nsym = 0, lg = 0;
				const int used = fse_read_ncount(d + p, avail - p, L.norm[t], max_sym, max_log, &nsym, &lg);
				if (used < 0) {
					err = 1;
				} else {
					p += (u32)used;
					spec = (u32)nsym | (u32)lg << 8;
				}
			}
			if ((want >> t) & 1)
				L.misc[ZM_A + t] = spec;
		}
		L.misc[ZM_ERR] = err;
		L.misc[ZM_E] = p;
	}
	wv_sync();
	return L.misc[ZM_ERR] == 0;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_pre_entropy_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			    const ZPre *__restrict__ pre, const u32 *__restrict__ def, u8 *__restrict__ slots,
			    u32 *__restrict__ mark)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	const int lane = wv_lane();
	const u32 b = blockIdx.x;
	if (lane < 36)
		L.llx[lane] = Z_LL_BASE[lane] | (u32)Z_LL_BITS[lane] << 24;
	if (lane < 53)
		L.mlx[lane] = Z_ML_BASE[lane] | (u32)Z_ML_BITS[lane] << 24;
	if (b >= nblk)
		return;
	const ZPre P = pre[b];
	const ZBlock B = blocks[b];
	if (!P.ok || B.src_off > stream_bytes || B.src_len > stream_bytes - B.src_off || P.bsize != B.src_len - 3 ||
	    B.block_max > Z_BLOCK_MAX || P.regen > B.block_max)
		return; /* (the mark is 0 since the classify kernel) */
	const u8 *mem_lo = stream, *mem_hi = stream + stream_bytes + 256;
	const u8 *src = stream + B.src_off + 3;
	const u32 bsize = P.bsize, regen = P.regen, lcsz = P.lcsz;
	const u32 ltype = P.lit & 3, nstreams = (P.lit >> 2) & 7, lhl = P.lit >> 8;
	u8 *lit_slot = slots + (size_t)b * Z_PRE_STRIDE;
	u64 *seq_slot = (u64 *)(lit_slot + Z_PRE_LIT);
	u32 m = 0;

	/* ================= literals ================= */
	if (ltype < 2) {
		m |= ZPRE_LIT; /* raw: read in place; RLE: a fill -- both stay with the execute stage */
	} else {
		/* the tree: this block's, or (treeless) the one its definer describes */
		const u32 tb = ltype == 2 ? b : def[4 * (size_t)b];
		bool ok = tb <= b; /* (ZPRE_NONE is above every index) */
		ZPre T = P;
		const u8 *tsrc = src;
		if (ok && tb != b) {
			T = pre[tb];
			const ZBlock TB = blocks[tb];
			ok = T.ok && (T.lit & 3) == 2 && TB.src_off <= stream_bytes && TB.src_len <= stream_bytes - TB.src_off &&
			     T.bsize == TB.src_len - 3;
			tsrc = stream + TB.src_off + 3;
		}
		int huf_log = 0;
		u32 tree = 0;
		if (ok) {
			const u32 thl = T.lit >> 8;
			wv_sync();
			stage_load(L.stage, tsrc, 0, 256, 0, mem_lo, mem_hi, lane);
			wv_sync();
			if (lane == 0) {
				const u8 *d = L.stage;
				const u32 avail = T.lcsz < 256 - thl ? T.lcsz : 256 - thl;
				int nw = 0, lg = 0;
				const int used = huf_read_weights(d + thl, avail, L.w, &nw, &lg, (u32 *)L.sq[0], L.norm[0], L.next[0]);
				L.misc[ZM_ERR] = used < 0 || lg > 11;
				L.misc[ZM_F] = used < 0 ? 0u : (u32)used;
				L.misc[ZM_G] = (u32)nw;
				L.misc[ZM_H] = (u32)lg;
			}
			wv_sync();
			ok = L.misc[ZM_ERR] == 0;
		}
		if (ok) {
			huf_log = (int)L.misc[ZM_H];
			tree = ltype == 2 ? L.misc[ZM_F] : 0u;
			for (u32 i = (u32)lane; i < (1u << 11); i += 64)
				L.huf[i] = 0;
			wv_sync();
			huf_fill(L.huf, L.w, (int)L.misc[ZM_G], huf_log, lane);
			wv_sync();
			ok = lcsz >= tree + (nstreams == 4 ? 10u : 1u);
		}
		/* ---- Huffman streams: lane s < nstreams decodes stream s (the walk of zstd_dec_body) ---- */
		const u32 body = lhl + tree;
		u32 s_off = body, s_len = lcsz - tree, s_n = regen, s_dst = 0;
		if (ok && nstreams == 4) {
			const u32 j1 = uld16(src + body), j2 = uld16(src + body + 2), j3 = uld16(src + body + 4);
			const u32 tot = lcsz - tree - 6, q = (regen + 3) / 4;
			if (j1 + j2 + j3 >= tot || 3 * q > regen) {
				ok = false;
			} else {
				const u32 sl = lane & 3;
				s_off = body + 6 + (sl > 0 ? j1 : 0) + (sl > 1 ? j2 : 0) + (sl > 2 ? j3 : 0);
				s_len = sl == 0 ? j1 : sl == 1 ? j2 : sl == 2 ? j3 : tot - j1 - j2 - j3;
				s_n = sl < 3 ? q : regen - 3 * q;
				s_dst = sl * q;
			}
		}
		if (ok) {
			const bool dec = (u32)lane < nstreams;
			bool bad = false;
			long pos = 0;
			if (dec) {
				const u32 lastb = s_len ? src[s_off + s_len - 1] : 0;
				if (s_len == 0 || lastb == 0)
					bad = true;
				else
					pos = 8 * (long)(s_len - 1) + hb32(lastb);
			}
			u32 done = 0;
			while (!wv_any(dec && bad) && wv_any(dec && done < s_n)) {
				wv_sync();
				{
					const int sg = lane >> 4;
					const u32 g_off = wv_shfl(s_off, sg);
					const u32 g_poslo = wv_shfl((u32)pos, sg);
					const u32 g_poshi = wv_shfl((u32)((u64)pos >> 32), sg);
					const long g_pos = (long)((u64)g_poshi << 32 | g_poslo);
					const long whi = (g_pos + 7) >> 3;
					if ((u32)sg < nstreams) {
						const u32 o = 16u * ((u32)lane & 15);
						const long rel = whi - 256 + (long)o;
						const u8 *p = src + g_off + rel;
						u64 a = 0, c = 0;
						if (rel >= 0 && p + 16 <= mem_hi) {
							a = ld64u(p);
							c = ld64u(p + 8);
						} else {
							for (int k = 0; k < 8; k++) {
								if (rel + k >= 0 && p + k < mem_hi)
									a |= (u64)p[k] << (8 * k);
								if (rel + 8 + k >= 0 && p + 8 + k < mem_hi)
									c |= (u64)p[8 + k] << (8 * k);
							}
						}
						u8 *w = L.stage + 256u * (u32)sg + o;
						*(u64 *)w = a;
						*(u64 *)(w + 8) = c;
					}
				}
				wv_sync();
				if (dec && done < s_n) {
					const u8 *win = L.stage + 256u * (u32)lane;
					const long wlo = ((pos + 7) >> 3) - 256;
					const u32 todo = s_n - done < 128 ? s_n - done : 128;
					u8 *dst = lit_slot + s_dst + done;
					const int lg = huf_log;
					const u32 hm = (1u << lg) - 1;
					int ipos = (int)pos;
					const int iwlo = (int)wlo;
					u32 i = 0;
					for (; i + 8 <= todo && ipos >= 0; i += 8) {
						u64 acc = 0;
						ZMT_UNROLL
						for (int hlf = 0; hlf < 2; hlf++) {
							const int tb2 = (ipos - 1) >> 3;
							const u64 word = ld64u(win + (tb2 - 7 - iwlo));
							int cb = ipos - 8 * (tb2 - 7);
							ZMT_UNROLL
							for (int k = 0; k < 4; k++) {
								const u32 e = L.huf[(u32)(word >> (cb - lg)) & hm];
								cb -= (int)(e >> 8);
								acc |= (u64)(e & 255) << (8 * (4 * hlf + k));
							}
							ipos = cb + 8 * (tb2 - 7);
						}
						st64g(dst + i, acc);
					}
					{
						u64 c = 0;
						int cb = 0;
						for (; i < todo && ipos >= 0; i++) {
							if (cb < lg) {
								const int tb2 = (ipos - 1) >> 3;
								c = ld64u(win + (tb2 - 7 - iwlo));
								cb = ipos - 8 * (tb2 - 7);
							}
							const u32 e = L.huf[(u32)(c >> (cb - lg)) & hm];
							const int nb = (int)(e >> 8);
							cb -= nb;
							ipos -= nb;
							dst[i] = (u8)e;
						}
					}
					if (ipos < 0)
						bad = true;
					pos = ipos;
					done += todo;
					if (!bad && done == s_n && pos != 0)
						bad = true;
				}
			}
			if (!wv_any(dec && bad))
				m |= ZPRE_LIT;
		}
	}

	/* ================= sequences ================= */
	const u32 nseq = P.nseq;
	if (nseq == 0) {
		m |= ZPRE_SEQ; /* nothing to decode */
	} else if (nseq <= Z_PRE_SEQCAP(B.block_max)) {
		const u32 modes = P.sqh >> 8;
		/* where each table comes from */
		u32 from[3];
		bool ok = true;
		for (int t = 0; t < 3; t++) {
			from[t] = ((modes >> (6 - 2 * t)) & 3) == 3 ? def[4 * (size_t)b + 1 + t] : b;
			if (from[t] > b) {
				ok = false;
			} else if (from[t] != b) {
				const ZPre D = pre[from[t]];
				const ZBlock DB = blocks[from[t]];
				if (!D.ok || D.nseq == 0 || (((D.sqh >> 8) >> (6 - 2 * t)) & 3) == 3 || DB.src_off > stream_bytes ||
				    DB.src_len > stream_bytes - DB.src_off || D.bsize != DB.src_len - 3)
					ok = false;
			}
		}
		int my_tab_log = 0;
		u32 sq_hdr = 0;
		/* this block first (its header also says where the bitstream starts), then the definers it names */
		for (int k = 0; k < 4 && ok; k++) {
			const u32 sb = k == 0 ? b : from[k - 1];
			u32 want = 0;
			for (int t = 0; t < 3; t++)
				if (from[t] == sb)
					want |= 1u << t;
			if (k > 0 && (sb == b || (k > 1 && from[0] == sb) || (k > 2 && from[1] == sb)))
				continue; /* built already */
			if (k > 0 && !want)
				continue;
			const ZPre D = k == 0 ? P : pre[sb];
			ok = zpre_seq_header(L, stream + blocks[sb].src_off + 3, D, want, mem_lo, mem_hi, lane);
			if (!ok)
				break;
			if (k == 0)
				sq_hdr = L.misc[ZM_E];
			bool terr = false;
			if (lane < 3 && ((want >> lane) & 1)) {
				const u32 spec = L.misc[ZM_A + lane];
				u32 *cells = lane == 0 ? L.ll : lane == 1 ? L.of : L.ml;
				if (spec == 0xFFFFFFFFu) {
					terr = true;
				} else if (spec & 0x80000000u) {
					const u32 sy = spec & 255;
					cells[0] = sy | (lane == 1 ? sy : (lane == 0 ? L.llx[sy] : L.mlx[sy]) >> 24) << 10;
					my_tab_log = 0;
				} else {
					const int lg = (int)((spec >> 8) & 255);
					terr = lg > (lane == 1 ? 8 : 9) ||
					       fse_build(cells, L.norm[lane], (int)(spec & 255), lg, L.next[lane],
							 lane == 0 ? L.llx : lane == 2 ? L.mlx : (const u32 *)nullptr, lane) != 0;
					my_tab_log = lg;
				}
			}
			wv_sync();
			if (wv_any(terr))
				ok = false;
		}
		const u32 bs_off = P.sq0 + sq_hdr;
		long pos = 0;
		if (ok && bs_off >= bsize)
			ok = false;
		if (ok) {
			const u32 bs_len = bsize - bs_off;
			const u32 lastb = uld8(src + bs_off + bs_len - 1);
			if (lastb == 0)
				ok = false;
			else
				pos = 8 * (long)(bs_len - 1) + hb32(lastb);
		}
		if (ok) {
			const int ll_log = (int)wv_readlane((u32)my_tab_log, 0), of_log = (int)wv_readlane((u32)my_tab_log, 1),
				  ml_log = (int)wv_readlane((u32)my_tab_log, 2);
			const u32 *mytab = lane == 1 ? L.of : lane == 2 ? L.ml : L.ll;
			u64 *myval = L.sq[lane < 3 ? lane : 0];
			const u32 e_of = lane == 1 ? 0u : ~0u, e_ml = lane == 0 ? ~0u : 0u;
			const u32 s_ll = lane == 0 ? 0u : ~0u, s_ml = lane == 1 ? ~0u : 0u;
			u32 state = 0;
			for (u32 sbase = 0; sbase < nseq && ok; sbase += 64) {
				const u32 k = nseq - sbase < 64 ? nseq - sbase : 64;
				const long whi = (pos + 7) >> 3, wlo = whi - (long)Z_STAGE;
				wv_sync();
				stage_load(L.stage, src + bs_off, wlo, Z_STAGE, -(long)(bs_off + 16), mem_lo, mem_hi, lane);
				wv_sync();
				const u8 *win = L.stage - wlo;
				if (sbase == 0) {
					if (pos < (long)(ll_log + of_log + ml_log)) {
						ok = false;
						break;
					}
					const long tb = (pos - 1) >> 3;
					const u64 w0 = ld64u(win + tb - 7), w1 = ld64u(win + tb - 15);
					const u32 skip = (u32)(8 * (tb + 1) - pos);
					state = xbits(w0, w1, skip + (lane == 0 ? 0u : lane == 1 ? (u32)ll_log : (u32)(ll_log + of_log)),
						      (u32)(lane < 3 ? my_tab_log : 0));
					pos -= ll_log + of_log + ml_log;
				}
				int bp = (int)pos;
				const u8 *winb = win - 15;
				for (u32 i = 0; i < k; i++) {
					const int tb = (bp - 1) >> 3;
					u64 w1 = 0, w0 = 0;
					if (lane < 3) {
						w1 = ld64u(winb + tb);
						w0 = ld64u(winb + tb + 8);
					}
					const u32 cell = mytab[state];
					const u32 skip = (u32)(8 * (tb + 1) - bp);
					const u32 nb = sbase + i + 1 == nseq ? 0u : ZC_NB(cell), ab = ZC_AB(cell);
					const u32 pk = ab | nb << 8;
					const u32 p_ll = wv_readlane(pk, 0), p_of = wv_readlane(pk, 1), p_ml = wv_readlane(pk, 2);
					const u32 a_ll = p_ll & 255, n_ll = p_ll >> 8, a_of = p_of & 255, n_of = p_of >> 8;
					const u32 a_ml = p_ml & 255, n_ml = p_ml >> 8;
					const u32 base3 = skip + a_of + a_ml + a_ll;
					const u32 eo = skip + (a_of & e_of) + (a_ml & e_ml);
					const u32 so = base3 + (n_ll & s_ll) + (n_ml & s_ml);
					const u32 extra = xbits(w0, w1, eo, ab);
					const u32 sbits = xbits(w0, w1, so, nb);
					if (lane < 3)
						myval[i] = (u64)extra | (u64)ZC_SYM(cell) << 32;
					state = lane < 3 ? ZC_BASE(cell) + sbits : 0;
					bp -= (int)(base3 - skip + n_ll + n_ml + n_of);
				}
				pos = bp;
				if (pos < 0 || (sbase + k == nseq && pos != 0)) {
					ok = false;
					break;
				}
				wv_sync();
				bool fit = true;
				if ((u32)lane < k) {
					const u64 q_ll = L.sq[0][lane], q_of = L.sq[1][lane], q_ml = L.sq[2][lane];
					const u32 c_of = (u32)(q_of >> 32);
					const u32 ll = (L.llx[(u32)(q_ll >> 32)] & 0xFFFFFFu) + (u32)q_ll;
					const u32 ml = (L.mlx[(u32)(q_ml >> 32)] & 0xFFFFFFu) + (u32)q_ml;
					/* offset codes above 27 do not fit the packing (and above 31 are an error): left to the block itself */
					fit = c_of <= 27;
					const u32 ofv = fit ? (1u << c_of) + (u32)q_of : 0u;
					seq_slot[sbase + (u32)lane] = (u64)ll | (u64)ml << 18 | (u64)ofv << 36;
				}
				if (wv_any(!fit))
					ok = false;
			}
			if (ok)
				m |= ZPRE_SEQ;
		}
	}
	if (lane == 0)
		mark[b] = m;
}

extern "C" __global__ void __launch_bounds__(64)
zmt_zstd_dec_run_pre_kernel(const u8 *__restrict__ stream, u64 stream_bytes, const ZBlock *__restrict__ blocks, u32 nblk,
			    const ZRun *__restrict__ runs, u32 nrun, u8 *out_base, u64 out_bytes, u8 *carry,
			    u32 *__restrict__ run_len, u32 *__restrict__ status, u8 *__restrict__ litbuf,
			    const u32 *__restrict__ mark, const u32 *__restrict__ def, const u8 *__restrict__ slots)
{
	__shared__ __attribute__((aligned(16))) ZLds L;
	zstd_dec_body<false, ZLds, true, true>(L, 0u, stream, stream_bytes, nullptr, nullptr, nrun, out_base, nullptr, run_len,
					       litbuf, status, nullptr, nullptr, nullptr, nullptr, 0, blocks, nblk, runs, out_bytes,
					       carry, mark, def, slots);
}

#include "zstd_dec_par.h"
#include "zstd_dec_rec.h"

/* ------------------------------------------------------------------ XXH64 content checksum
 * Four lanes per record = the four accumulators of XXH64 (one 32-byte stripe per step); only records
 * that carry a checksum do any work. */
#define X64_1 0x9E3779B185EBCA87ull
#define X64_2 0xC2B2AE3D27D4EB4Full
#define X64_3 0x165667B19E3779F9ull
#define X64_4 0x85EBCA77C2B2AE63ull
#define X64_5 0x27D4EB2F165667C5ull
static __device__ __forceinline__ u64 rotl64(u64 x, int r) { return (x << r) | (x >> (64 - r)); }
static __device__ __forceinline__ u64 x64_round(u64 acc, u64 in) { return rotl64(acc + in * X64_2, 31) * X64_1; }
static __device__ __forceinline__ u64 x64_merge(u64 h, u64 v) { return (h ^ x64_round(0, v)) * X64_1 + X64_4; }
static __device__ __forceinline__ u64 shfl64(u64 v, int src)
{
	return (u64)wv_shfl((u32)(v >> 32), src) << 32 | wv_shfl((u32)v, src);
}

extern "C" __global__ void __launch_bounds__(256)
zmt_xxh64_verify_kernel(const u8 *__restrict__ base, const u64 *__restrict__ off,
			const u32 *__restrict__ len, u32 n, const u32 *__restrict__ expect,
			const u32 *__restrict__ valid, u32 *__restrict__ status)
{
	const u32 gtid = blockIdx.x * 256 + threadIdx.x;
	const u32 item = gtid >> 2, a = gtid & 3;
	const int lane = wv_lane();
	const bool live = item < n && valid[item] && status[item] == ST_OK;
	const u8 *p = live ? base + off[item] : base;
	const u32 N = live ? len[item] : 0;
	u64 v = a == 0 ? X64_1 + X64_2 : a == 1 ? X64_2 : a == 2 ? 0ull : 0ull - X64_1;
	if (N >= 32) {
		const u8 *q = p + 8 * a;
		for (u32 s = 0; s < (N >> 5); s++) {
			v = x64_round(v, ld64u(q));
			q += 32;
		}
	}
	/* all four accumulators to lane 0 of the quad (wave-uniform shuffles) */
	const int q0 = lane & ~3;
	const u64 v1 = shfl64(v, q0), v2 = shfl64(v, q0 + 1), v3 = shfl64(v, q0 + 2), v4 = shfl64(v, q0 + 3);
	if (live && a == 0) {
		u64 h;
		if (N >= 32) {
			h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
			h = x64_merge(h, v1);
			h = x64_merge(h, v2);
			h = x64_merge(h, v3);
			h = x64_merge(h, v4);
		} else {
			h = X64_5;
		}
		h += N;
		const u8 *t = p + (N & ~31u), *e = p + N;
		for (; t + 8 <= e; t += 8)
			h = rotl64(h ^ x64_round(0, ld64u(t)), 27) * X64_1 + X64_4;
		if (t + 4 <= e) {
			h = rotl64(h ^ (u64)ld32u(t) * X64_1, 23) * X64_2 + X64_3;
			t += 4;
		}
		for (; t < e; t++)
			h = rotl64(h ^ (u64)*t * X64_5, 11) * X64_1;
		h ^= h >> 33;
		h *= X64_2;
		h ^= h >> 29;
		h *= X64_3;
		h ^= h >> 32;
		if ((u32)h != expect[item])
			status[item] = ST_BAD_CHECKSUM;
	}
}

/* out_len[i] = Frame_Content_Size of record i (what the host needs before it can size d_out);
 * status[i] = ST_OK, or why the record cannot be decoded here. */
extern "C" __global__ void __launch_bounds__(256)
zmt_zstd_probe_kernel(const u8 *__restrict__ stream, const u64 *__restrict__ rec_off,
		      const u32 *__restrict__ rec_len, u32 nrec, u32 *__restrict__ out_len,
		      u32 *__restrict__ status)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nrec)
		return;
	const u8 *r = stream + rec_off[i];
	const u32 rlen = rec_len[i];
	u32 st = ST_OK, n = 0;
	if (rlen < 18 || ld32u(r) != ZMT_SKIP_MAGIC || ld32u(r + 4) != 4 || ld32u(r + 8) != rlen - 12) {
		st = ST_BAD_RECORD;
	} else if (ld32u(r + 12) != ZMT_ZSTD_MAGIC) {
		st = ST_BAD_FRAME;
	} else {
		const u8 *f = r + 12;
		const u32 flen = rlen - 12, fhd = f[4], fcs = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
		const u32 did_len = did == 3 ? 4 : did, fcs_len = fcs == 0 ? single : (1u << fcs);
		const u32 hp = 5 + (1 - single) + did_len;
		if ((fhd & 8) || flen < hp + fcs_len) {
			st = ST_BAD_FRAME;
		} else if (fcs_len == 0) {
			st = ST_UNSUPPORTED; /* no content size: never written by zstd-mt (one-shot ZSTD_compress) */
		} else {
			u64 c = 0;
			for (u32 k = 0; k < fcs_len; k++)
				c |= (u64)f[hp + k] << (8 * k);
			if (fcs == 1)
				c += 256;
			if (c > 0x7FFFFFFFull)
				st = ST_UNSUPPORTED;
			else
				n = (u32)c;
		}
	}
	out_len[i] = n;
	status[i] = st;
}

/*
 * XXH64 (seed 0) with carried state (gpumt_xxh64_carry): the content checksum of a plain .zst frame that is decoded run
 * after run, as zmt_xxh32_carry_kernel (xxh32.hip) is for .lz4.  One wave per job: lanes 0..3 run the four accumulators
 * over the 32-byte stripes, the up to 31 bytes that do not fill a stripe wait in the state.  A state is 20 words in device
 * memory: acc[4] (lo, hi), total length (lo, hi), pending count, spare, 32 pending bytes.  Jobs of one launch run side by
 * side, so the one that reads a carried state and the one that leaves one name different slots.  Same job record and flags
 * as the XXH32 call; `expect` is compared with the low 32 bits, which is what a zstd frame stores.
 */
struct Xxh64Job { /* == gpumt_xxh32_job */
	u64 off;
	u32 len, flags, expect, reserved;
};
#define X64J_RESET 1u
#define X64J_FINAL 2u
#define X64J_VERIFY 4u
#define X64J_IN(f) (((f) >> 8) & 1u)
#define X64J_OUT(f) (((f) >> 9) & 1u)
#define X64_STATE_WORDS 20

extern "C" __global__ void __launch_bounds__(64)
zmt_xxh64_carry_kernel(const u8 *__restrict__ base, u64 base_bytes, const Xxh64Job *__restrict__ jobs, u32 njobs,
		       u32 *__restrict__ states, u32 *__restrict__ digest, u32 *__restrict__ verdict)
{
	__shared__ __attribute__((aligned(8))) u8 tail[32];
	const u32 j = blockIdx.x;
	const int lane = wv_lane();
	if (j >= njobs)
		return;
	const Xxh64Job J = jobs[j];
	if (J.off > base_bytes || J.len > base_bytes - J.off) {
		if (lane == 0) {
			digest[j] = 0;
			verdict[j] = ST_BAD_RECORD;
		}
		return;
	}
	const u32 a = (u32)lane & 3;
	const u32 *sin = states + X64_STATE_WORDS * X64J_IN(J.flags);
	u32 *sout = states + X64_STATE_WORDS * X64J_OUT(J.flags);
	u64 acc = a == 0 ? X64_1 + X64_2 : a == 1 ? X64_2 : a == 2 ? 0ull : 0ull - X64_1;
	u32 npend = 0;
	u64 total = 0;
	if (!(J.flags & X64J_RESET)) {
		acc = (u64)sin[2 * a] | (u64)sin[2 * a + 1] << 32;
		total = (u64)sin[8] | (u64)sin[9] << 32;
		npend = sin[10] & 31u;
		if (lane < 8)
			*(u32 *)(tail + 4 * lane) = sin[12 + lane];
	}
	wv_sync();
	const u8 *p = base + J.off;
	u32 len = J.len;
	total += len;
	/* complete the pending stripe first: byte k of it is byte k - npend of the piece */
	if (npend) {
		const u32 take = 32 - npend < len ? 32 - npend : len;
		if ((u32)lane >= npend && (u32)lane < npend + take)
			tail[lane] = p[(u32)lane - npend];
		wv_sync();
		p += take;
		len -= take;
		npend += take;
		if (npend == 32) {
			acc = x64_round(acc, *(const u64 *)(tail + 8 * a));
			npend = 0;
		}
		wv_sync();
	}
	if (lane < 4) {
		const u8 *q = p + 8 * a;
		u32 ns = len >> 5, s = 0;
		for (; s + 8 <= ns; s += 8) {
			u64 x[8];
			for (u32 k = 0; k < 8; k++)
				x[k] = ld64u(q + 32 * k);
			for (u32 k = 0; k < 8; k++)
				acc = x64_round(acc, x[k]);
			q += 256;
		}
		for (; s < ns; s++) {
			acc = x64_round(acc, ld64u(q));
			q += 32;
		}
	}
	if (npend == 0) { /* (else the piece ended inside the pending stripe: len is 0) */
		npend = len & 31;
		if ((u32)lane < npend)
			tail[lane] = p[(len & ~31u) + (u32)lane];
	}
	wv_sync();
	if (J.flags & X64J_FINAL) {
		const u64 v1 = shfl64(acc, 0), v2 = shfl64(acc, 1), v3 = shfl64(acc, 2), v4 = shfl64(acc, 3);
		if (lane == 0) {
			u64 h;
			if (total >= 32) {
				h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
				h = x64_merge(h, v1);
				h = x64_merge(h, v2);
				h = x64_merge(h, v3);
				h = x64_merge(h, v4);
			} else {
				h = X64_5;
			}
			h += total;
			u32 t = 0;
			for (; t + 8 <= npend; t += 8)
				h = rotl64(h ^ x64_round(0, *(const u64 *)(tail + t)), 27) * X64_1 + X64_4;
			if (t + 4 <= npend) {
				h = rotl64(h ^ (u64)*(const u32 *)(tail + t) * X64_1, 23) * X64_2 + X64_3;
				t += 4;
			}
			for (; t < npend; t++)
				h = rotl64(h ^ (u64)tail[t] * X64_5, 11) * X64_1;
			h ^= h >> 33;
			h *= X64_2;
			h ^= h >> 29;
			h *= X64_3;
			h ^= h >> 32;
			digest[j] = (u32)h;
			verdict[j] = (J.flags & X64J_VERIFY) && (u32)h != J.expect ? ST_BAD_CHECKSUM : ST_OK;
		}
	} else {
		if (lane < 4) {
			sout[2 * a] = (u32)acc;
			sout[2 * a + 1] = (u32)(acc >> 32);
		}
		if (lane < 8)
			sout[12 + lane] = (u32)lane * 4 < npend ? *(const u32 *)(tail + 4 * lane) : 0u;
		if (lane == 0) {
			sout[8] = (u32)total;
			sout[9] = (u32)(total >> 32);
			sout[10] = npend;
			sout[11] = 0;
			digest[j] = 0;
			verdict[j] = ST_OK;
		}
	}
}

#ifdef ZMT_EMU
/* TEST HARNESS ONLY (tests/emu compiles this file as host C++): the two block-level calls over the fiber emulator, with
 * the shapes of include/gpumt.h, as the ones at the end of lz4_dec.hip and xxh32.hip.  Never part of the product. */
#include <vector>
#include "../../../include/gpumt.h"
extern "C" {
void emu_zstd_decompress_blocks(const u8 *stream, u64 stream_bytes, const void *blocks, u32 nblk, const void *runs, u32 nrun,
				u8 *out, u64 out_bytes, u8 *carry, u32 *run_len, u32 *status)
{
	std::vector<u8> lit((size_t)nrun * Z_RUN_LITSLOT, 0xA5); /* scratch starts as garbage */
	u8 *litp = lit.data();
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_zstd_dec_run_kernel(stream, stream_bytes, (const ZBlock *)blocks, nblk, (const ZRun *)runs, nrun, out, out_bytes,
					carry, run_len, status, litp);
	});
}

void emu_xxh64_carry(const u8 *base, u64 base_bytes, const void *jobs, u32 njobs, u32 *states, u32 *digest, u32 *verdict)
{
	emu::launch(emu::dim3{njobs, 1, 1}, emu::dim3{64, 1, 1},
		    [=]() { zmt_xxh64_carry_kernel(base, base_bytes, (const Xxh64Job *)jobs, njobs, states, digest, verdict); });
}

int gpumt_zstd_decompress_blocks(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const gpumt_zstd_block *d_blocks,
				 size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun, void *d_out, size_t out_bytes,
				 void *d_carry, uint32_t *d_run_len, uint32_t *d_status, int s)
{
	static_assert(sizeof(gpumt_zstd_block) == sizeof(ZBlock) && sizeof(gpumt_zstd_run) == sizeof(ZRun) &&
			      GPUMT_ZSTD_CARRY_BYTES == sizeof(ZCarry) && GPUMT_ZSTD_RUN_SCRATCH == Z_RUN_LITSLOT,
		      "table layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_stream || !d_blocks || !d_runs || !d_out || !d_carry || !d_run_len ||
	    !d_status || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX || stream_bytes > 0xFFFFFFF0u)
		return GPUMT_E_ARG;
	emu_zstd_decompress_blocks((const u8 *)d_stream, stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out,
				   out_bytes, (u8 *)d_carry, d_run_len, d_status);
	return GPUMT_OK;
}

/* pre_on = 0: the serial kernel, every mark 0 (the developer knob of the real boundary) */
void emu_zstd_decompress_blocks_pre(const u8 *stream, u64 stream_bytes, const void *blocks, u32 nblk, const void *runs,
				    u32 nrun, u8 *out, u64 out_bytes, u8 *carry, u32 *run_len, u32 *status, u32 *block_mark,
				    int pre_on)
{
	std::vector<u32> markv((size_t)nblk + 1, 0xA5A5A5A5u);
	if (!pre_on || nblk == 0) {
		emu_zstd_decompress_blocks(stream, stream_bytes, blocks, nblk, runs, nrun, out, out_bytes, carry, run_len, status);
		for (u32 i = 0; block_mark && i < nblk; i++)
			block_mark[i] = 0;
		return;
	}
	std::vector<u8> lit((size_t)nrun * Z_RUN_LITSLOT, 0xA5), slots((size_t)nblk * Z_PRE_STRIDE, 0xA5);
	std::vector<ZPre> prev(nblk);
	std::vector<u32> defv((size_t)nblk * 4, 0xA5A5A5A5u);
	u8 *litp = lit.data(), *slotp = slots.data();
	ZPre *prep = prev.data();
	u32 *defp = defv.data(), *markp = markv.data();
	emu::launch(emu::dim3{(nblk + 255) / 256, 1, 1}, emu::dim3{256, 1, 1}, [=]() {
		zmt_zstd_pre_classify_kernel(stream, stream_bytes, (const ZBlock *)blocks, nblk, prep, defp, markp);
	});
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{64, 1, 1},
		    [=]() { zmt_zstd_pre_resolve_kernel((const ZRun *)runs, nrun, nblk, prep, defp, nullptr); });
	emu::launch(emu::dim3{nblk, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_zstd_pre_entropy_kernel(stream, stream_bytes, (const ZBlock *)blocks, nblk, prep, defp, slotp, markp);
	});
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{64, 1, 1}, [=]() {
		zmt_zstd_dec_run_pre_kernel(stream, stream_bytes, (const ZBlock *)blocks, nblk, (const ZRun *)runs, nrun, out,
					    out_bytes, carry, run_len, status, litp, markp, defp, slotp);
	});
	for (u32 i = 0; block_mark && i < nblk; i++)
		block_mark[i] = markv[i];
}

int gpumt_zstd_decompress_blocks_pre(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const gpumt_zstd_block *d_blocks,
				     size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun, void *d_out, size_t out_bytes,
				     void *d_carry, uint32_t *d_run_len, uint32_t *d_status, uint32_t *d_block_mark, int s)
{
	static_assert(GPUMT_ZSTD_PRE_SCRATCH(Z_BLOCK_MAX) == Z_PRE_STRIDE && sizeof(ZPre) == 32, "table layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_stream || !d_blocks || !d_runs || !d_out || !d_carry || !d_run_len ||
	    !d_status || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX || stream_bytes > 0xFFFFFFF0u)
		return GPUMT_E_ARG;
	/* (the emulated boundary keeps no variants: the environment alone, read once and validated as gpumt_open does) */
	static int pre_on = -1;
	if (pre_on < 0) {
		const char *e = getenv("GPUMT_ZSTD_RUN_PRE");
		pre_on = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				pre_on = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_ZSTD_RUN_PRE=%s ignored (0 or 1)\n", e);
		}
	}
	emu_zstd_decompress_blocks_pre((const u8 *)d_stream, stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out,
				       out_bytes, (u8 *)d_carry, d_run_len, d_status, d_block_mark, pre_on);
	return GPUMT_OK;
}

/* par_on = 0: the pre call, every block_par 0 */
void emu_zstd_decompress_blocks_par(const u8 *stream, u64 stream_bytes, const void *blocks_, u32 nblk, const void *runs_,
				    u32 nrun, u8 *out, u64 out_bytes, u8 *carry, u32 *run_len, u32 *status, u32 *block_mark,
				    u32 *block_par, int par_on)
{
	for (u32 i = 0; block_par && i < nblk; i++)
		block_par[i] = 0;
	if (!par_on || nblk == 0) {
		emu_zstd_decompress_blocks_pre(stream, stream_bytes, blocks_, nblk, runs_, nrun, out, out_bytes, carry, run_len,
					       status, block_mark, 1);
		return;
	}
	const ZBlock *blocks = (const ZBlock *)blocks_;
	const ZRun *runs = (const ZRun *)runs_;
	std::vector<u8> lit((size_t)nrun * Z_RUN_LITSLOT, 0xA5), slots((size_t)nblk * Z_PRE_STRIDE, 0xA5);
	std::vector<ZPre> prev(nblk);
	std::vector<u32> defv((size_t)nblk * 4, 0xA5A5A5A5u), markv((size_t)nblk, 0xA5A5A5A5u), parv((size_t)nblk, 0);
	std::vector<u32> origin((size_t)out_bytes + 4, 0xA5A5A5A5u), perrun((size_t)nrun * 13, 0xA5A5A5A5u),
		perblk((size_t)nblk * 11 + 1, 0xA5A5A5A5u);
	std::vector<ZRun> prun(nrun);
	std::vector<u8> pcarry((size_t)nrun * sizeof(ZCarry), 0xA5);
	u8 *litp = lit.data(), *slotp = slots.data();
	ZPre *prep = prev.data();
	u32 *defp = defv.data(), *markp = markv.data(), *parp = parv.data();
	ZPar P;
	P.origin = origin.data();
	P.prun = prun.data();
	P.pcarry = pcarry.data();
	P.sfx = perrun.data();
	P.rflag = P.sfx + nrun;
	P.plen = P.rflag + nrun;
	P.pst = P.plen + nrun;
	P.rrep = P.pst + nrun;
	P.rlen = P.rrep + 3 * (size_t)nrun;
	P.rlast = P.rlen + nrun;
	P.owner = perblk.data();
	P.blen = P.owner + nblk;
	P.bst = P.blen + nblk;
	P.btf = P.bst + nblk;
	P.bpos = P.btf + 3 * (size_t)nblk;
	P.brep = P.bpos + nblk;
	P.xst = P.brep + 3 * (size_t)nblk;
	P.flag = P.xst + nblk;
	for (u32 i = 0; i < nblk; i++)
		P.owner[i] = ZPAR_NONE;
	P.flag[0] = 0;
	const emu::dim3 wave{64, 1, 1};
	emu::launch(emu::dim3{(nblk + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
		    [=]() { zmt_zstd_pre_classify_kernel(stream, stream_bytes, blocks, nblk, prep, defp, markp); });
	emu::launch(emu::dim3{nrun, 1, 1}, wave, [=]() { zmt_zstd_pre_resolve_kernel(runs, nrun, nblk, prep, defp, P.rlast); });
	emu::launch(emu::dim3{nblk, 1, 1}, wave,
		    [=]() { zmt_zstd_pre_entropy_kernel(stream, stream_bytes, blocks, nblk, prep, defp, slotp, markp); });
	emu::launch(emu::dim3{1, 1, 1}, wave, [=]() { zmt_zstd_par_plan_kernel(runs, nrun, nblk, out_bytes, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, wave,
		    [=]() { zmt_zstd_par_split_kernel(stream, stream_bytes, blocks, nblk, runs, nrun, out_bytes, markp, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, wave, [=]() {
		zmt_zstd_par_prefix_kernel(stream, stream_bytes, blocks, nblk, runs, nrun, out, out_bytes, carry, litp, markp, defp,
					   slotp, P);
	});
	emu::launch(emu::dim3{nblk, 1, 1}, wave,
		    [=]() { zmt_zstd_par_measure_kernel(stream, stream_bytes, blocks, nblk, runs, prep, markp, slotp, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, wave, [=]() { zmt_zstd_par_scan_kernel(runs, nrun, P); });
	emu::launch(emu::dim3{nblk, 1, 1}, wave,
		    [=]() { zmt_zstd_par_exec_kernel(stream, stream_bytes, blocks, nblk, runs, prep, slotp, out, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, emu::dim3{ZPAR_RESOLVE_THREADS, 1, 1},
		    [=]() { zmt_zstd_par_resolve_kernel(runs, nrun, out, P); });
	emu::launch(emu::dim3{nrun, 1, 1}, wave, [=]() {
		zmt_zstd_par_fallback_kernel(stream, stream_bytes, blocks, nblk, runs, nrun, out, out_bytes, carry, run_len, status,
					     litp, markp, defp, slotp, P);
	});
	emu::launch(emu::dim3{nrun, 1, 1}, wave, [=]() {
		zmt_zstd_par_carry_kernel(stream, stream_bytes, blocks, nblk, runs, nrun, prep, carry, run_len, status, parp, P);
	});
	for (u32 i = 0; i < nblk; i++) {
		if (block_mark)
			block_mark[i] = markv[i];
		if (block_par)
			block_par[i] = parv[i];
	}
}

int gpumt_zstd_decompress_blocks_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const gpumt_zstd_block *d_blocks,
				     size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun, void *d_out, size_t out_bytes,
				     void *d_carry, uint32_t *d_run_len, uint32_t *d_status, uint32_t *d_block_mark,
				     uint32_t *d_block_par, int s)
{
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_stream || !d_blocks || !d_runs || !d_out || !d_carry || !d_run_len ||
	    !d_status || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX || stream_bytes > 0xFFFFFFF0u)
		return GPUMT_E_ARG;
	/* (the environment alone, as the pre call above) */
	static int par_on = -1;
	if (par_on < 0) {
		const char *e = getenv("GPUMT_ZSTD_RUN_PAR");
		par_on = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				par_on = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_ZSTD_RUN_PAR=%s ignored (0 or 1)\n", e);
		}
	}
	if (!par_on) {
		for (size_t i = 0; d_block_par && i < nblk; i++)
			d_block_par[i] = 0;
		return gpumt_zstd_decompress_blocks_pre(h, d_stream, stream_bytes, d_blocks, nblk, d_runs, nrun, d_out, out_bytes,
							d_carry, d_run_len, d_status, d_block_mark, s);
	}
	emu_zstd_decompress_blocks_par((const u8 *)d_stream, stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out,
				       out_bytes, (u8 *)d_carry, d_run_len, d_status, d_block_mark, d_block_par, 1);
	return GPUMT_OK;
}

int gpumt_xxh64_carry(gpumt_ctx *h, const void *d_base, size_t base_bytes, const gpumt_xxh32_job *d_jobs, size_t njobs,
		      uint32_t *d_states, uint32_t *d_digest, uint32_t *d_verdict, int s)
{
	static_assert(sizeof(gpumt_xxh32_job) == sizeof(Xxh64Job) && GPUMT_XXH64_STATE_WORDS == X64_STATE_WORDS, "table layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || !d_base || !d_jobs || !d_states || !d_digest || !d_verdict ||
	    njobs > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (njobs)
		emu_xxh64_carry((const u8 *)d_base, base_bytes, d_jobs, (u32)njobs, d_states, d_digest, d_verdict);
	return GPUMT_OK;
}

/* the record decoders over the emulator (tests/emu/emu_api.cpp) */
void emu_zstd_decompress_batch(const u8 *stream, u64 stream_bytes, const u64 *rec_off, const u32 *rec_len, u32 nrec, u8 *out,
			       const u64 *out_off, u32 *out_len, u32 *status);

/* gpumt_zstd_decompress_batch_par with its knobs as arguments (cap_mb: 0 = none); stats (may be NULL) receives what the
 * trace line of the real boundary prints: records, par, blocks, slices, fallback */
void emu_zstd_decompress_batch_par(const u8 *stream, u64 stream_bytes, const u64 *rec_off, const u32 *rec_len, u32 nrec, u8 *out,
				   u64 out_bytes, const u64 *out_off, u32 *out_len, u32 *status, u32 *rec_par, u32 min_blocks,
				   u32 slice_blocks, int par_on, u32 cap_mb, u32 *stats)
{
	u32 st5[5] = {nrec, 0, 0, 0, 0};
	for (u32 i = 0; rec_par && i < nrec; i++)
		rec_par[i] = 0;
	if (!par_on) {
		emu_zstd_decompress_batch(stream, stream_bytes, rec_off, rec_len, nrec, out, out_off, out_len, status);
		if (stats)
			memcpy(stats, st5, sizeof st5);
		return;
	}
	std::vector<ZRec> recv(nrec);
	std::vector<u32> sst(status, status + nrec), ce(nrec, 0xA5A5A5A5u), cv(nrec, 0), rfv(nrec, 0xA5A5A5A5u), rrv(nrec, 0xA5A5A5A5u);
	ZRec *recs = recv.data();
	u32 *sstp = sst.data(), *cep = ce.data(), *cvp = cv.data(), *rfp = rfv.data(), *rrp = rrv.data();
	emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1}, [=]() {
		zmt_zstd_rec_count_kernel(stream, stream_bytes, rec_off, rec_len, nrec, out_off, out_len, out_bytes, status,
					  min_blocks, recs);
	});
	ZRecSlice S;
	/* the scratch the real boundary would ask for: per record, and the largest slice's tables */
	size_t max_blk = 0, max_run = 0, nslices = 0;
	for (size_t at = 0; zrec_next_slice(recs, nrec, at, slice_blocks, &S); at = S.b) {
		max_blk = S.nblk > max_blk ? S.nblk : max_blk;
		max_run = S.nrun > max_run ? S.nrun : max_run;
		nslices++;
	}
	const size_t need = (size_t)nrec * (sizeof(ZRec) + 20) + max_blk * sizeof(ZBlock) + max_run * (sizeof(ZRun) + 8) +
			    2 * sizeof(ZCarry);
	if (!nslices || (cap_mb && need > ((size_t)cap_mb << 20))) {
		st5[4] = nslices ? 1 : 0;
		emu_zstd_decompress_batch(stream, stream_bytes, rec_off, rec_len, nrec, out, out_off, out_len, status);
		if (stats)
			memcpy(stats, st5, sizeof st5);
		return;
	}
	for (size_t at = 0; zrec_next_slice(recs, nrec, at, slice_blocks, &S); at = S.b) {
		const u32 n = (u32)(S.b - S.a), nblk = S.nblk, nrun = S.nrun;
		std::vector<ZBlock> blkv(nblk);
		std::vector<ZRun> runv(nrun);
		std::vector<u32> rlv(nrun, 0xA5A5A5A5u), rsv(nrun, 99u);
		std::vector<u8> cyv(2 * sizeof(ZCarry), 0xA5);
		ZBlock *blk = blkv.data();
		ZRun *run = runv.data();
		u32 *rl = rlv.data(), *rs = rsv.data();
		const ZRec *sr = recs + S.a;
		u32 *sf = rfp + S.a, *sn = rrp + S.a;
		const u64 in_lo = S.in_lo, out_lo = S.out_lo;
		emu::launch(emu::dim3{1, 1, 1}, emu::dim3{256, 1, 1}, [=]() { zmt_zstd_rec_scan_kernel(sr, n, sf, sn); });
		emu::launch(emu::dim3{(n + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
			    [=]() { zmt_zstd_rec_table_kernel(stream, sr, n, sf, sn, in_lo, out_lo, nblk, nrun, blk, run); });
		emu_zstd_decompress_blocks_par(stream + S.in_lo, S.in_hi - S.in_lo, blk, nblk, run, nrun, out + S.out_lo,
					       S.out_hi - S.out_lo, cyv.data(), rl, rs, nullptr, nullptr, 1);
		u32 *ol = out_len + S.a, *rp = rec_par ? rec_par + S.a : nullptr, *ss = sstp + S.a, *e = cep + S.a, *v = cvp + S.a;
		emu::launch(emu::dim3{(n + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
			    [=]() { zmt_zstd_rec_finish_kernel(stream, sr, n, sn, nrun, rl, rs, ol, rp, ss, e, v); });
		st5[1] += nrun;
		st5[2] += nblk;
		st5[3]++;
	}
	/* the record decoders judge everything the block stages did not keep (their own checksum pass included) */
	emu_zstd_decompress_batch(stream, stream_bytes, rec_off, rec_len, nrec, out, out_off, out_len, sstp);
	emu::launch(emu::dim3{(nrec + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
		    [=]() { zmt_zstd_rec_merge_kernel(sstp, nrec, status); });
	emu::launch(emu::dim3{(nrec * 4 + 255) / 256, 1, 1}, emu::dim3{256, 1, 1},
		    [=]() { zmt_xxh64_verify_kernel(out, out_off, out_len, nrec, cep, cvp, status); });
	if (stats)
		memcpy(stats, st5, sizeof st5);
}

static int emu_rec_env(const char *name, int lo, int hi, int dflt)
{
	const char *e = getenv(name);
	if (!e || !*e)
		return dflt;
	char *end;
	const long v = strtol(e, &end, 10);
	if (*end || v < lo || v > hi) {
		fprintf(stderr, "gpumt: %s=%s ignored (%d..%d)\n", name, e, lo, hi);
		return dflt;
	}
	return (int)v;
}

int gpumt_zstd_decompress_batch_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				    const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				    const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int s)
{
	static_assert(sizeof(ZRec) == 56, "record layout");
	if (!h || s < 0 || s >= GPUMT_NSTREAMS || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	/* (the environment alone, as the block calls above; read once, by whichever thread comes first: the initialisation of
	 * a function-local static is synchronised) */
	struct Knobs {
		int min_blocks, slice_blocks, trace;
		Knobs()
		{
			const char *e = getenv("GPUMT_TRACE");
			trace = e && *e ? atoi(e) : 0;
			slice_blocks = emu_rec_env("GPUMT_ZSTD_REC_SLICE_BLOCKS", 2, 65536, 4096);
			min_blocks = emu_rec_env("GPUMT_ZSTD_REC_MIN_BLOCKS", 1, 65536, 4);
		}
	};
	static const Knobs knobs;
	const int min_blocks = knobs.min_blocks, slice_blocks = knobs.slice_blocks, trace = knobs.trace;
	u32 st5[5];
	emu_zstd_decompress_batch_par((const u8 *)d_stream, stream_bytes, d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, out_bytes,
				      d_out_off, d_out_len, d_status, d_rec_par, (u32)min_blocks, (u32)slice_blocks, 1, 0, st5);
	if (trace >= 1)
		fprintf(stderr, "[gpumt zstd rec] records %u par %u blocks %u slices %u fallback %u\n", st5[0], st5[1], st5[2], st5[3],
			st5[4]);
	return GPUMT_OK;
}
}
#endif
