/*
 * gpumt.hip -- C-ABI shim between the plain-C host engine and the gfx950 kernels (include/gpumt.h).
 * Owns the HIP device, four streams, timing events and per-handle scratch; launches the kernels.
 * There is deliberately no CPU fallback anywhere in this file.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/gpumt.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

/* record layout and slice rule of gpumt_zstd_decompress_batch_par */
#define ZREC_HOST_ONLY
#include "zstd_dec_rec.h"
/* ... and of gpumt_lz4_decompress_batch_par */
#define LREC_HOST_ONLY
#include "lz4_dec_rec.h"
/* ... and of gpumt_brotli_decompress_batch_par */
#define BREC_HOST_ONLY
#include "brotli_dec_rec.h"

extern "C" {
__global__ void zmt_xxh32_kernel(const u8 *, const u64 *, const u32 *, u32, u32 *, const u32 *,
				 const u32 *, u32 *);
__global__ void zmt_lz4_enc3_u16_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					unsigned long long *);
__global__ void zmt_lz4_enc3_p17_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					unsigned long long *);
__global__ void zmt_lz4_enc3_p17_prof_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					     unsigned long long *);
__global__ void zmt_push_host_kernel(const u8 *, u8 *, u64, const u64 *);
__global__ void zmt_lz4hc_enc_kernel(const u8 *, u64, u32, u32, u8 *, u64, u32 *, const u32 *, u8 *, int);
__global__ void zmt_lz4_enc5_u16_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					unsigned long long *);
__global__ void zmt_lz4_enc5_p17_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					unsigned long long *);
__global__ void zmt_lz4_enc5_u32_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					unsigned long long *);
__global__ void zmt_lz4_enc3_u32_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *,
					unsigned long long *);
__global__ void zmt_lz4_dec_serial(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *,
				   u32 *, u32 *, u32 *, u32 *, u32);
__global__ void zmt_lz4_dec_serial_kept(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *,
					u32 *, u32 *, u32 *, u32 *, u32, const u32 *);
/* scratch of gpumt_zstd_decompress_blocks_par (zstd_dec_par.h) */
struct ZPar {
	u32 *origin;
	gpumt_zstd_run *prun;
	u8 *pcarry;
	u32 *sfx, *rflag, *plen, *pst, *rrep, *rlen, *rlast, *owner, *blen, *bst, *btf, *bpos, *brep, *xst, *flag;
};
__global__ void zmt_zstd_par_plan_kernel(const gpumt_zstd_run *, u32, u32, u64, ZPar);
__global__ void zmt_zstd_par_split_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, u32, u64,
					  const u32 *, ZPar);
__global__ void zmt_zstd_par_prefix_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, u32, u8 *,
					   u64, const u8 *, u8 *, const u32 *, const u32 *, const u8 *, ZPar);
__global__ void zmt_zstd_par_measure_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *,
					    const void *, const u32 *, const u8 *, ZPar);
__global__ void zmt_zstd_par_scan_kernel(const gpumt_zstd_run *, u32, ZPar);
__global__ void zmt_zstd_par_exec_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, const void *,
					 u8 *, u8 *, ZPar);
__global__ void zmt_zstd_par_resolve_kernel(const gpumt_zstd_run *, u32, u8 *, ZPar);
__global__ void zmt_zstd_par_fallback_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, u32, u8 *,
					     u64, u8 *, u32 *, u32 *, u8 *, const u32 *, const u32 *, const u8 *, ZPar);
__global__ void zmt_zstd_par_carry_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, u32,
					  const void *, u8 *, u32 *, u32 *, u32 *, ZPar);
/* the record stage in front of it (zstd_dec_rec.h) */
__global__ void zmt_zstd_rec_count_kernel(const u8 *, u64, const u64 *, const u32 *, u32, const u64 *, const u32 *, u64,
					  const u32 *, u32, ZRec *);
__global__ void zmt_zstd_rec_scan_kernel(const ZRec *, u32, u32 *, u32 *);
__global__ void zmt_zstd_rec_table_kernel(const u8 *, const ZRec *, u32, const u32 *, const u32 *, u64, u64, u32, u32,
					  gpumt_zstd_block *, gpumt_zstd_run *);
__global__ void zmt_zstd_rec_finish_kernel(const u8 *, const ZRec *, u32, const u32 *, u32, const u32 *, const u32 *, u32 *,
					   u32 *, u32 *, u32 *, u32 *);
__global__ void zmt_zstd_rec_merge_kernel(const u32 *, u32, u32 *);
/* scratch of gpumt_lz4_decompress_blocks_par (lz4_dec_par.h) */
struct Lz4Par {
	u16 *origin;
	u32 *owner, *mlen, *mst, *pos, *xst, *flag;
};
__global__ void zmt_lz4_par_plan_kernel(const gpumt_lz4_run *, u32, u32, u64, Lz4Par);
__global__ void zmt_lz4_par_measure_kernel(const u8 *, u64, const gpumt_lz4_block *, u32, Lz4Par);
__global__ void zmt_lz4_par_scan_kernel(const u8 *, u64, const gpumt_lz4_block *, u32, const gpumt_lz4_run *, u32, u8 *, u64,
					u32 *, u32 *, u32 *, Lz4Par);
__global__ void zmt_lz4_par_exec_kernel(const u8 *, const gpumt_lz4_block *, u32, const gpumt_lz4_run *, u8 *, Lz4Par);
__global__ void zmt_lz4_par_resolve_kernel(const gpumt_lz4_run *, u32, u32, u8 *, u64, u32 *, u32 *, u32 *, Lz4Par);
/* scratch of gpumt_lz4_decompress_blocks_seg (lz4_dec_seg.h) */
struct Lz4Seg {
	u16 *origin;
	u32 *owner, *mlen, *mst, *pos, *nseg, *cbase, *cut, *xst, *flag;
	u32 shift, ncut;
};
__global__ void zmt_lz4_seg_plan_kernel(const gpumt_lz4_block *, u32, const gpumt_lz4_run *, u32, u64, Lz4Seg);
__global__ void zmt_lz4_seg_measure_kernel(const u8 *, u64, const gpumt_lz4_block *, u32, Lz4Seg);
__global__ void zmt_lz4_seg_scan_kernel(const u8 *, u64, const gpumt_lz4_block *, u32, const gpumt_lz4_run *, u32, u8 *, u64,
					u32 *, u32 *, u32 *, Lz4Seg);
__global__ void zmt_lz4_seg_exec_kernel(const u8 *, const gpumt_lz4_block *, u32, const gpumt_lz4_run *, u8 *, Lz4Seg);
__global__ void zmt_lz4_seg_resolve_kernel(const gpumt_lz4_run *, u32, u32, u8 *, u64, u32 *, u32 *, u32 *, u32 *, Lz4Seg);
/* the record stage in front of the two (lz4_dec_rec.h) */
__global__ void zmt_lz4_rec_count_kernel(const u8 *, u64, const u64 *, const u32 *, u32, const u64 *, const u32 *, u64, u32,
					 u32, LRec *);
__global__ void zmt_lz4_rec_scan_kernel(const LRec *, u32, u32 *, u32 *);
__global__ void zmt_lz4_rec_table_kernel(const u8 *, const LRec *, u32, const u32 *, const u32 *, u64, u64, u32, u32,
					 gpumt_lz4_block *, gpumt_lz4_run *);
__global__ void zmt_lz4_rec_finish_kernel(const u8 *, const LRec *, u32, const u32 *, u32, const u32 *, const u32 *, u32 *,
					  u32 *, u32 *, u32 *, u32 *);
__global__ void zmt_lz4_rec_merge_kernel(const u32 *, u32, u32 *, u32 *);
__global__ void zmt_lz4_dec_blocks_kernel(const u8 *, u64, const gpumt_lz4_block *, u32, const gpumt_lz4_run *, u32, u8 *,
					  u64, u32 *, u32 *, u32 *);
__global__ void zmt_lz4_gather_runs_kernel(const u8 *, u64, const gpumt_lz4_run *, const u32 *, const u64 *, u32, u8 *,
					   u64);
__global__ void zmt_xxh32_carry_kernel(const u8 *, u64, const gpumt_xxh32_job *, u32, u32 *, u32 *, u32 *);
__global__ void zmt_dec_nblk_kernel(const u32 *, u32, u32 *);
__global__ void zmt_dec_frames_kernel(const u8 *, const u64 *, const u32 *, u32, const u32 *,
				      const u64 *, u64 *, u32 *, u32 *, u32 *, u32 *, u32 *, u32 *);
__global__ void zmt_dec_frames_kept_kernel(const u8 *, const u64 *, const u32 *, u32, const u32 *,
					   const u64 *, u64 *, u32 *, u32 *, u32 *, u32 *, u32 *, u32 *, const u32 *);
__global__ void zmt_dec_parse4_kernel(const u8 *, u64, const u64 *, const u32 *, const u64 *, u16 *, u32 *, u32 *);
#define C3_DECL(NAME)                                                                                              \
	__global__ void NAME(const u8 *, u64, u32, u32, u8 *, const u64 *, const u32 *, const u64 *, const u64 *,  \
			     const u32 *, const u32 *, const u32 *, const u16 *, const u32 *, const u32 *, u32 *);
C3_DECL(zmt_dec_copy3_w4_kernel)
C3_DECL(zmt_dec_copy3_w8_kernel)
C3_DECL(zmt_dec_copy3_w16_kernel)
#define C3_DECLP(NAME)                                                                                             \
	__global__ void NAME(const u8 *, u64, u32, u32, u8 *, const u64 *, const u32 *, const u64 *, const u64 *,  \
			     const u32 *, const u32 *, const u32 *, const u16 *, const u32 *, const u32 *, u32 *, \
			     unsigned long long *);
C3_DECLP(zmt_dec_copy3_w4_kernel_prof)
C3_DECLP(zmt_dec_copy3_w8_kernel_prof)
C3_DECLP(zmt_dec_copy3_w16_kernel_prof)
__global__ void zmt_brotli_enc_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *);
__global__ void zmt_brotli_enc_t2_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *);
__global__ void zmt_brotli_enc_t3_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *);
__global__ void zmt_snappy_enc_kernel(const u8 *, u64, u32, u32, u8 *, u64, u32 *);
__global__ void zmt_snappy_dec_kernel(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *, const u32 *, u32 *, u32 *);
__global__ void zmt_snappy_dec2_kernel(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *, const u32 *, u32 *, u32 *);
__global__ void zmt_brotli_enc_win_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *, const u32 *, u32);
__global__ void zmt_brotli_assemble_kernel(u64, u32, u32, u32, u8 *, u64, const u32 *, u32 *);
__global__ void zmt_brotli_assemble_index_kernel(u64, u32, u32, u32, u8 *, u64, const u32 *, u32 *);
__global__ void zmt_brotli_rec_plan_kernel(const u8 *, const u64 *, const u32 *, u32, const u64 *, const u32 *, u32, BRec *);
__global__ void zmt_brotli_rec_scan_kernel(const BRec *, u32, u32 *);
__global__ void zmt_brotli_rec_table_kernel(const u8 *, const BRec *, u32, u32, const u32 *, u32, B4Span *);
__global__ void zmt_brotli_rec_finish_kernel(const BRec *, u32, const u32 *, u32, const B4Span *, const u32 *, u32 *, u32 *, u32 *);
__global__ void zmt_brotli_dec4_wanted_kernel(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *, const u32 *,
					      u32 *, u32 *, u32);
__global__ void zmt_brotli_dec4_span_kernel(const u8 *, const B4Span *, u32, u8 *, u32 *);
__global__ void zmt_brotli_dec_kernel(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *, const u32 *,
				      u32 *, u32 *, u8 *, const u8 *, u32);
__global__ void zmt_brotli_dec_kernel_prof(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *,
					   const u32 *, u32 *, u32 *, u8 *, const u8 *, u32, unsigned long long *);
#ifndef B4_NG
#define B4_NG 4 /* streams per wave of zmt_brotli_dec4_kernel (brotli_dec4.hip) */
#endif
__global__ void zmt_brotli_dec4_kernel(const u8 *, const u64 *, const u32 *, u32, u8 *, const u64 *, const u32 *,
				       u32 *, u32 *);
__global__ void zmt_zstd_dec_small_kernel(const u8 *, u64, const u64 *, const u32 *, u32, u8 *, const u64 *,
					  u32 *, u8 *, u32 *, u32 *, u32 *, u8 *, u64);
__global__ void zmt_zstd_dec_kernel(const u8 *, u64, const u64 *, const u32 *, u32, u8 *, const u64 *,
				    u32 *, u8 *, u32 *, u32 *, u32 *, u32, u8 *, u64);
__global__ void zmt_zstd_dec_kernel_prof(const u8 *, u64, const u64 *, const u32 *, u32, u8 *, const u64 *,
					 u32 *, u8 *, u32 *, u32 *, u32 *, u32, unsigned long long *, u8 *, u64);
__global__ void zmt_zstd_seq_kernel(const u8 *, u64, const u64 *, const u32 *, u32, const u64 *, const u32 *,
				    const u32 *, u8 *, u64);
__global__ void zmt_zstd_dec_run_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, u32, u8 *,
					u64, u8 *, u32 *, u32 *, u8 *);
__global__ void zmt_zstd_pre_classify_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, void *, u32 *, u32 *);
__global__ void zmt_zstd_pre_resolve_kernel(const gpumt_zstd_run *, u32, u32, const void *, u32 *, u32 *);
__global__ void zmt_zstd_pre_entropy_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const void *, const u32 *, u8 *,
					    u32 *);
__global__ void zmt_zstd_dec_run_pre_kernel(const u8 *, u64, const gpumt_zstd_block *, u32, const gpumt_zstd_run *, u32, u8 *,
					    u64, u8 *, u32 *, u32 *, u8 *, const u32 *, const u32 *, const u8 *);
__global__ void zmt_xxh64_carry_kernel(const u8 *, u64, const gpumt_xxh32_job *, u32, u32 *, u32 *, u32 *);
__global__ void zmt_xxh64_verify_kernel(const u8 *, const u64 *, const u32 *, u32, const u32 *, const u32 *,
					u32 *);
__global__ void zmt_zstd_enc_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *);
__global__ void zmt_zstd_enc_t2_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *);
__global__ void zmt_zstd_enc_t3_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *);
__global__ void zmt_zstd_enc_kernel_prof(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *, unsigned long long *);
__global__ void zmt_zstd_win_chain_kernel(const u8 *, u64, u32, u32, u32 *, u32 *);
__global__ void zmt_win_chain_seg_kernel(const u8 *, u64, u32, u32, u32, u32, u32, u32 *, u32 *);
__global__ void zmt_win_chain_carry_kernel(u64, u32, u32, u32, u32, u32, u32 *);
__global__ void zmt_win_chain_patch_kernel(const u8 *, u64, u32, u32, u32, u32, u32 *, const u32 *);
__global__ void zmt_zstd_enc_win_kernel(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, u8 *, const u32 *, u32);
__global__ void zmt_zstd_assemble_kernel(u64, u32, u32, u32, u8 *, u64, const u32 *, u32 *);
__global__ void zmt_zstd_probe_kernel(const u8 *, const u64 *, const u32 *, u32, u32 *, u32 *);
__global__ void zmt_probe_kernel(const u8 *, const u64 *, const u32 *, u32, u32 *);
__global__ void zmt_scan_kernel(const u32 *, u32, u64 *);
__global__ void zmt_compact_kernel(const u8 *, u64, const u32 *, const u64 *, u32, u8 *);
__global__ void zmt_iota_kernel(u64 *, u32 *, u64, u64, u32);
}

#define NTIMERS 16

struct gpumt_ctx {
	int device;
	hipStream_t st[GPUMT_NSTREAMS];
	hipEvent_t t0[NTIMERS], t1[NTIMERS];
	hipEvent_t xev;
	hipEvent_t mark[GPUMT_NMARKS];
	/* scratch, grown on demand (never shrinks) */
	void *scratch[2][GPUMT_NSTREAMS]; /* [0] compress side, [1] decompress side; one per launching stream, so
					   * batches launched on different streams can overlap */
	size_t scratch_bytes[2][GPUMT_NSTREAMS];
	int dec_variant;
	unsigned long long *d_prof; /* 16 phase counters of the profiling decoder */
	int xflags;  /* experiment switches of the parse kernel (developer) */
	int lz4_ring; /* copy3: log2 of the LDS ring per wave (12, 13 or 14) */
	int enc_variant; /* LZ4 fast levels: 0 = the window encoder (lz4_enc5.hip), 3 = the probe-batch encoder (lz4_enc3.hip) */
	int dec_pad;  /* copy stage: dynamic-LDS padding per workgroup = resident-wave cap (developer A/B, GPUMT_LZ4_DEC_PAD) */
	int debug_free; /* GPUMT_DEBUG_FREE: gpumt_free / gpumt_host_free check that the streams are idle */
	int profile; /* record events in timer slots 8.. around individual kernels */
	int num_cus;
	int zenc_waves[3]; /* resident waves of the persistent zstd encoder kernels (whole device), per level tier */
	int zwin_waves;   /* ... of the whole-chunk-window encoder (gpumt_zstd_compress_batch_win) */
	int zwin_depth;   /* its candidates per position: 0 = by level (gpumt_zstd_win_depth), 1..256 = this many (A/B runs) */
	int zwin_cap_mb;  /* 0 = none; else scratch requests of that call above this many MiB count as refused (the tests' way to the fallback) */
	size_t zwin_refused; /* the smallest scratch of that call the device has refused (0 = none yet): not asked for again */
	int bwin_waves;   /* the same four of the brotli encoder's window (gpumt_brotli_compress_batch_win, gpumt_brotli_win_depth) */
	int bwin_depth;
	int bwin_cap_mb;
	size_t bwin_refused;
	int wchain_par;   /* the chain plane of both: 0 = one wave per chunk, 1 = in segments of the default size, 12..24 = of 1 << that many positions */
	int wchain_cap_mb; /* 0 = none; else head tables of the segment build above this many MiB count as refused (the tests' way to the fallback) */
	size_t wchain_refused; /* the smallest head tables the device has refused (0 = none yet): not asked for again */
	int wchain_waves; /* resident waves of the segment kernel (whole device) */
	int trace;        /* GPUMT_TRACE */
	int hc_waves;     /* developer: grid of the LZ4HC encoder (0 = GPUMT_LZ4HC_WAVES) */
	int zdec_variant; /* 0 = small-table kernel, then general; 1 = general only */
	int zseq_variant; /* 0 = sequence pre-pass (zstd_dec_seq.hip) in front of the frame decoder; 1 = none */
	int zrun_pre;     /* 1 = entropy pre-pass in front of the block runs (gpumt_zstd_decompress_blocks_pre); 0 = none */
	size_t zrun_pre_refused; /* the smallest pre-pass scratch the device has refused (0 = none yet): not asked for again */
	int zrun_par;     /* 1 = block-parallel execute stage behind it (gpumt_zstd_decompress_blocks_par); 0 = none */
	size_t zrun_par_refused; /* the same for that stage's scratch */
	int zrec_par;     /* 1 = multi-block records through the block stages (gpumt_zstd_decompress_batch_par); 0 = the record decoders alone */
	int zrec_min_blocks;   /* records of fewer blocks stay with the record decoders */
	int zrec_slice_blocks; /* blocks per call of the block stages */
	int zrec_cap_mb;  /* 0 = none; else that stage's own scratch above this many MiB counts as refused (the tests' way to the fallback) */
	size_t zrec_refused; /* the smallest such scratch the device has refused (0 = none yet): not asked for again */
	void *zrec_area[GPUMT_NSTREAMS]; /* that stage's own device scratch: the block calls and the record decoders replace scratch[1] */
	size_t zrec_bytes[GPUMT_NSTREAMS];
	void *zrec_tab[GPUMT_NSTREAMS];  /* ... and its tables per slice, sized once the counts are known */
	size_t zrec_tab_bytes[GPUMT_NSTREAMS];
	void *zrec_pin[GPUMT_NSTREAMS]; /* pinned copy of the per-record counts, for the host to cut slices */
	size_t zrec_pin_bytes[GPUMT_NSTREAMS];
	int lrun_par;     /* 1 = linked runs of plain .lz4 blocks side by side (gpumt_lz4_decompress_blocks_par); 0 = one wave per run */
	size_t lrun_par_refused; /* the smallest origin-plane scratch the device has refused (0 = none yet): not asked for again */
	int lblk_seg;     /* 1 = plain .lz4 blocks in segments side by side (gpumt_lz4_decompress_blocks_seg); 0 = one wave per run */
	int lseg_bytes;   /* the segment of that call: a power of two, 256 .. 4 MiB */
	size_t lblk_seg_refused; /* the same for that call's scratch */
	int lrec_par;     /* 1 = multi-block lz4-mt records through the block calls (gpumt_lz4_decompress_batch_par); 0 = the record decoders alone */
	int lrec_seg;     /* 0 = gpumt_lz4_decompress_blocks_par decodes the slices, 1 = gpumt_lz4_decompress_blocks_seg */
	int lrec_min_blocks;   /* records of fewer parts stay with the record decoders */
	int lrec_slice_blocks; /* blocks per call of the block stages */
	int lrec_cap_mb;  /* 0 = none; else that stage's own scratch above this many MiB counts as refused (the tests' way to the fallback) */
	size_t lrec_refused; /* the smallest such scratch the device has refused (0 = none yet): not asked for again */
	void *lrec_area[GPUMT_NSTREAMS]; /* that stage's own device scratch: the block calls and the record decoders replace scratch[1] */
	size_t lrec_bytes[GPUMT_NSTREAMS];
	void *lrec_tab[GPUMT_NSTREAMS];  /* ... and its tables per slice, sized once the counts are known */
	size_t lrec_tab_bytes[GPUMT_NSTREAMS];
	void *lrec_pin[GPUMT_NSTREAMS]; /* pinned copy of the per-record counts, for the host to cut slices */
	size_t lrec_pin_bytes[GPUMT_NSTREAMS];
	/* the same of gpumt_brotli_decompress_batch_par (brotli_dec_rec.h) */
	int brec_par;       /* 1 = indexed brotli-mt records span by span; 0 = the record decoders alone */
	int brec_min_spans; /* records of fewer spans stay with the record decoders */
	int brec_cap_mb;
	size_t brec_refused;
	void *brec_area[GPUMT_NSTREAMS]; /* per record: the plan and the first span */
	size_t brec_bytes[GPUMT_NSTREAMS];
	void *brec_tab[GPUMT_NSTREAMS]; /* per slice: the span table and a status word per span */
	size_t brec_tab_bytes[GPUMT_NSTREAMS];
	void *brec_pin[GPUMT_NSTREAMS];
	size_t brec_pin_bytes[GPUMT_NSTREAMS];
	int sdec_variant; /* snappy decoder: 0 = element by element, 1 = 64 elements per batch (snappy.hip) */
	int bdec_variant; /* brotli decoder: 0 = by batch size, 1 = the general kernel only, 2 = dec4 (four records per wave) + general for what it hands over */
	int bdec_waves;   /* resident waves of the persistent brotli decoder kernel (whole device) */
	int benc_waves[3]; /* resident waves of the persistent brotli encoder kernels (whole device), per quality tier */
	int senc_waves, sdec_waves, sdec2_waves; /* ... of the snappy kernels */
	void *d_brotli_static; /* device copy of the RFC 7932 constant data */
	char err[256];
	char name[128];
};

static int fail(gpumt_ctx *h, hipError_t e, const char *what)
{
	if (h)
		snprintf(h->err, sizeof h->err, "%s: %s", what, hipGetErrorString(e));
	return GPUMT_E_HIP;
}
#define CK(call)                                                                                   \
	do {                                                                                       \
		hipError_t e_ = (call);                                                            \
		if (e_ != hipSuccess)                                                              \
			return fail(h, e_, #call);                                                 \
	} while (0)

#define PROF0(slot)                                                                               \
	do {                                                                                       \
		if (h->profile)                                                                    \
			(void)hipEventRecord(h->t0[slot], h->st[s]);                               \
	} while (0)
#define PROF1(slot)                                                                               \
	do {                                                                                       \
		if (h->profile)                                                                    \
			(void)hipEventRecord(h->t1[slot], h->st[s]);                               \
	} while (0)

static int use(gpumt_ctx *h)
{
	CK(hipSetDevice(h->device));
	return GPUMT_OK;
}

static void *dev_alloc(gpumt_ctx *h, size_t bytes);
static void dev_free(gpumt_ctx *h, void *p);

static int want_scratch(gpumt_ctx *h, int k, int s, size_t bytes)
{
	if (bytes <= h->scratch_bytes[k][s])
		return GPUMT_OK;
	if (h->scratch[k][s]) {
		/* only work queued on this stream can be using the old area; a device-wide wait here would
		 * stall the batches other slots have in flight (130 ms per growing brotli batch, GPUMT_TRACE) */
		CK(hipStreamSynchronize(h->st[s]));
		dev_free(h, h->scratch[k][s]);
		h->scratch[k][s] = NULL;
		h->scratch_bytes[k][s] = 0;
	}
	bytes = (bytes + 0xFFFFF) & ~(size_t)0xFFFFF;
	h->scratch[k][s] = dev_alloc(h, bytes);
	if (!h->scratch[k][s]) {
		snprintf(h->err, sizeof h->err, "device scratch of %zu bytes: out of memory", bytes);
		return GPUMT_E_HIP;
	}
	h->scratch_bytes[k][s] = bytes;
	return GPUMT_OK;
}

extern "C" {

int gpumt_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

/* The host engines keep several batches in flight on streams of their own; with the runtime's default of 4
 * hardware queues those streams share queues and wait for each other's kernels (measured:
 * tools/ubench/pipe_overlap.hip).  Set once, when the library is loaded -- before any thread of the host can be
 * inside getenv / setenv on our account and before the first HIP call of a process that reaches HIP through
 * this library (the CLI, the drop-in APIs); a host that exports its own value, or initialised HIP earlier, keeps
 * what it has (overwrite = 0). */
__attribute__((constructor)) static void gpumt_library_init(void) { setenv("GPU_MAX_HW_QUEUES", "16", 0); }

int gpumt_open(int device, gpumt_ctx **out)
{
	int n = 0;
	gpumt_ctx *h;
	if (!out)
		return GPUMT_E_ARG;
	*out = NULL;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
		return GPUMT_E_NODEVICE;
	if (device == GPUMT_DEVICE_DEFAULT) {
		/* the drop-in APIs (LZ4MT_* ...) have no device argument: GPUMT_DEVICE selects the GPU of
		 * the contexts a process creates (one process per GPU, like the ranks of bench.py) */
		const char *e = getenv("GPUMT_DEVICE");
		device = (e && *e) ? atoi(e) : 0;
	}
	if (device < 0 || device >= n)
		return GPUMT_E_NODEVICE;
	h = (gpumt_ctx *)calloc(1, sizeof *h);
	if (!h)
		return GPUMT_E_NOMEM;
	h->device = device;
	{
		hipDeviceProp_t p;
		hipError_t e = hipSetDevice(device);
		if (e == hipSuccess)
			e = hipGetDeviceProperties(&p, device);
		if (e != hipSuccess) {
			free(h);
			return GPUMT_E_NODEVICE;
		}
		snprintf(h->name, sizeof h->name, "%s (%s, %d CUs)", p.name, p.gcnArchName,
			 p.multiProcessorCount);
		h->num_cus = p.multiProcessorCount;
		if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
			/* kernels are built for gfx950 only */
			free(h);
			return GPUMT_E_NODEVICE;
		}
	}
	for (int i = 0; i < GPUMT_NSTREAMS; i++)
		if (hipStreamCreateWithFlags(&h->st[i], hipStreamNonBlocking) != hipSuccess) {
			free(h);
			return GPUMT_E_HIP;
		}
	for (int i = 0; i < NTIMERS; i++) {
		(void)hipEventCreate(&h->t0[i]);
		(void)hipEventCreate(&h->t1[i]);
	}
	(void)hipEventCreateWithFlags(&h->xev, hipEventDisableTiming);
	for (int i = 0; i < GPUMT_NMARKS; i++)
		(void)hipEventCreateWithFlags(&h->mark[i], hipEventDisableTiming);
	{
		/* developer knob for A/B runs through the drop-in API / the CLI, which have no handle to call
		 * gpumt_set_variant on: GPUMT_SNAPPY_DEC=1 selects the batched snappy decoder */
		const char *e = getenv("GPUMT_SNAPPY_DEC");
		h->sdec_variant = e && *e ? atoi(e) : 0;
		/* GPUMT_LZ4_DEC: 0 = frames + parse4 + copy3 (default), 1 = frame-serial;
		 * GPUMT_LZ4_RING: log2 of copy3's LDS ring per wave (12 = 4 KiB, the default; 13; 14) */
		e = getenv("GPUMT_LZ4_DEC");
		h->dec_variant = e && *e ? atoi(e) : 0;
		e = getenv("GPUMT_LZ4_RING");
		h->lz4_ring = e && *e ? atoi(e) : 12;
		e = getenv("GPUMT_LZ4_ENC");
		h->enc_variant = e && *e ? atoi(e) : 0;
		e = getenv("GPUMT_LZ4_DEC_PAD");
		h->dec_pad = e && *e ? atoi(e) : 0;
		/* GPUMT_ZSTD_SEQ=1: no sequence pre-pass in front of the zstd frame decoder */
		e = getenv("GPUMT_ZSTD_SEQ");
		h->zseq_variant = e && *e ? atoi(e) : 0;
		/* GPUMT_ZSTD_RUN_PRE=0: gpumt_zstd_decompress_blocks_pre decodes serially, without its entropy pre-pass */
		e = getenv("GPUMT_ZSTD_RUN_PRE");
		h->zrun_pre = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				h->zrun_pre = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_ZSTD_RUN_PRE=%s ignored (0 or 1)\n", e);
		}
		/* GPUMT_ZSTD_RUN_PAR=0: gpumt_zstd_decompress_blocks_par decodes as gpumt_zstd_decompress_blocks_pre */
		e = getenv("GPUMT_ZSTD_RUN_PAR");
		h->zrun_par = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				h->zrun_par = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_ZSTD_RUN_PAR=%s ignored (0 or 1)\n", e);
		}
		/* gpumt_zstd_decompress_batch_par: GPUMT_ZSTD_REC_MIN_BLOCKS (1..65536) and GPUMT_ZSTD_REC_SLICE_BLOCKS (2..65536) */
		h->zrec_par = 1;
		h->zrec_min_blocks = 4;
		h->zrec_slice_blocks = 4096;
		for (int k = 0; k < 2; k++) {
			const char *name = k ? "GPUMT_ZSTD_REC_SLICE_BLOCKS" : "GPUMT_ZSTD_REC_MIN_BLOCKS";
			e = getenv(name);
			if (e && *e) {
				char *end;
				const long v = strtol(e, &end, 10);
				if (*end || v < (k ? 2 : 1) || v > 65536)
					fprintf(stderr, "gpumt: %s=%s ignored (%d..65536)\n", name, e, k ? 2 : 1);
				else
					*(k ? &h->zrec_slice_blocks : &h->zrec_min_blocks) = (int)v;
			}
		}
		/* GPUMT_LZ4_RUN_PAR=0: gpumt_lz4_decompress_blocks_par decodes every run with one wave */
		e = getenv("GPUMT_LZ4_RUN_PAR");
		h->lrun_par = 1;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				h->lrun_par = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_LZ4_RUN_PAR=%s ignored (0 or 1)\n", e);
		}
		/* GPUMT_LZ4_BLOCK_SEG=0: gpumt_lz4_decompress_blocks_seg decodes every run with one wave */
		e = getenv("GPUMT_LZ4_BLOCK_SEG");
		h->lblk_seg = 1;
		h->lseg_bytes = 65536;
		if (e && *e) {
			if ((e[0] == '0' || e[0] == '1') && !e[1])
				h->lblk_seg = e[0] - '0';
			else
				fprintf(stderr, "gpumt: GPUMT_LZ4_BLOCK_SEG=%s ignored (0 or 1)\n", e);
		}
		/* gpumt_lz4_decompress_batch_par: GPUMT_LZ4_REC_SEG (0 or 1), GPUMT_LZ4_REC_MIN_BLOCKS and
		 * GPUMT_LZ4_REC_SLICE_BLOCKS (2..65536) */
		h->lrec_par = 1;
		h->lrec_seg = 0;
		h->lrec_min_blocks = 4096; /* profiles/lz4_rec_par.txt */
		h->lrec_slice_blocks = 4096;
		for (int k = 0; k < 3; k++) {
			const char *name = k == 0 ? "GPUMT_LZ4_REC_SEG" : k == 1 ? "GPUMT_LZ4_REC_MIN_BLOCKS" : "GPUMT_LZ4_REC_SLICE_BLOCKS";
			const long lo = k ? 2 : 0, hi = k ? 65536 : 1;
			e = getenv(name);
			if (e && *e) {
				char *end;
				const long v = strtol(e, &end, 10);
				if (*end || v < lo || v > hi)
					fprintf(stderr, "gpumt: %s=%s ignored (%ld..%ld)\n", name, e, lo, hi);
				else
					*(k == 0 ? &h->lrec_seg : k == 1 ? &h->lrec_min_blocks : &h->lrec_slice_blocks) = (int)v;
			}
		}
		/* gpumt_brotli_decompress_batch_par: GPUMT_BROTLI_REC_MIN_SPANS (2..65536) */
		h->brec_par = 1;
		h->brec_min_spans = 2; /* profiles/brotli_rec_par.txt */
		e = getenv("GPUMT_BROTLI_REC_MIN_SPANS");
		if (e && *e) {
			char *end;
			const long v = strtol(e, &end, 10);
			if (*end || v < 2 || v > 65536)
				fprintf(stderr, "gpumt: GPUMT_BROTLI_REC_MIN_SPANS=%s ignored (2..65536)\n", e);
			else
				h->brec_min_spans = (int)v;
		}
		/* GPUMT_WIN_CHAIN_PAR: the window encoders' chain plane in segments (gpumt_set_variant "win_chain_par": 1 or
		 * 12..24); unset, empty and any other text = off */
		e = getenv("GPUMT_WIN_CHAIN_PAR");
		if (e && *e) {
			char *end;
			const long v = strtol(e, &end, 10);
			if (!*end && (v == 1 || (v >= 12 && v <= 24)))
				h->wchain_par = (int)v;
		}
		e = getenv("GPUMT_TRACE");
		h->trace = e && *e ? atoi(e) : 0;
		/* GPUMT_BROTLI_DEC: 0 = the batch size chooses (default), 1 = the general kernel, 2 = dec4 first */
		e = getenv("GPUMT_BROTLI_DEC");
		h->bdec_variant = e && *e ? atoi(e) : 0;
		/* GPUMT_DEBUG_FREE=1: the guard of the buffer contract (include/gpumt.h) for callers without a handle */
		e = getenv("GPUMT_DEBUG_FREE");
		h->debug_free = e && *e ? atoi(e) : 0;
		if (h->debug_free)
			fprintf(stderr, "gpumt: free guard on for device %d (GPUMT_DEBUG_FREE)\n", device);
	}
	*out = h;
	return GPUMT_OK;
}

void gpumt_close(gpumt_ctx *h)
{
	if (!h)
		return;
	(void)hipSetDevice(h->device);
	(void)hipDeviceSynchronize();
	for (int k = 0; k < 2; k++)
		for (int i = 0; i < GPUMT_NSTREAMS; i++)
			if (h->scratch[k][i])
				dev_free(h, h->scratch[k][i]);
	for (int i = 0; i < GPUMT_NSTREAMS; i++) {
		if (h->zrec_area[i])
			dev_free(h, h->zrec_area[i]);
		if (h->zrec_tab[i])
			dev_free(h, h->zrec_tab[i]);
		if (h->zrec_pin[i])
			(void)hipHostFree(h->zrec_pin[i]);
		if (h->lrec_area[i])
			dev_free(h, h->lrec_area[i]);
		if (h->lrec_tab[i])
			dev_free(h, h->lrec_tab[i]);
		if (h->lrec_pin[i])
			(void)hipHostFree(h->lrec_pin[i]);
		if (h->brec_area[i])
			dev_free(h, h->brec_area[i]);
		if (h->brec_tab[i])
			dev_free(h, h->brec_tab[i]);
		if (h->brec_pin[i])
			(void)hipHostFree(h->brec_pin[i]);
	}
	for (int i = 0; i < NTIMERS; i++) {
		(void)hipEventDestroy(h->t0[i]);
		(void)hipEventDestroy(h->t1[i]);
	}
	(void)hipEventDestroy(h->xev);
	for (int i = 0; i < GPUMT_NMARKS; i++)
		(void)hipEventDestroy(h->mark[i]);
	for (int i = 0; i < GPUMT_NSTREAMS; i++)
		(void)hipStreamDestroy(h->st[i]);
	free(h);
}

const char *gpumt_last_error(gpumt_ctx *h) { return h ? h->err : "no handle"; }
const char *gpumt_device_name(gpumt_ctx *h) { return h ? h->name : ""; }

int gpumt_host_node(gpumt_ctx *h)
{
	char bus[64] = "", path[128];
	int node = -1;
	if (!h || hipDeviceGetPCIBusId(bus, (int)sizeof bus, h->device) != hipSuccess)
		return -1;
	for (char *c = bus; *c; c++)
		if (*c >= 'A' && *c <= 'F')
			*c = (char)(*c - 'A' + 'a'); /* sysfs spells the address in lower case */
	snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
	FILE *f = fopen(path, "r");
	if (!f)
		return -1;
	if (fscanf(f, "%d", &node) != 1)
		node = -1;
	fclose(f);
	return node;
}

/*
 * Device buffers of a context (batch slots, per-wave scratch) are GiB-sized and hipMalloc / hipFree of
 * that size cost tens of milliseconds each -- 0.86 s of a 1.3 s BROTLIMT_decompressDCtx call on 8 GiB
 * were first-use allocations (GPUMT_TRACE).  Like the pinned staging buffers below, freed device
 * buffers therefore stay in a process-wide cache (per device, bounded by GPUMT_DEVICE_CACHE_MB,
 * default 16384) for the next context of the process.
 */
#define DEV_CACHE_SLOTS 192
static struct {
	pthread_mutex_t mu;
	void *p[DEV_CACHE_SLOTS];
	size_t cap[DEV_CACHE_SLOTS];
	int dev[DEV_CACHE_SLOTS];
	int used[DEV_CACHE_SLOTS];
	size_t idle, limit;
	int init;
} g_dev = {PTHREAD_MUTEX_INITIALIZER, {0}, {0}, {0}, {0}, 0, 0, 0};

static void *dev_alloc(gpumt_ctx *h, size_t bytes)
{
	void *p = NULL;
	int slot = -1;
	if (!bytes)
		bytes = 1;
	pthread_mutex_lock(&g_dev.mu);
	if (!g_dev.init) {
		const char *e = getenv("GPUMT_DEVICE_CACHE_MB");
		g_dev.limit = (size_t)(e && *e ? strtoull(e, 0, 10) : 16384) << 20;
		g_dev.init = 1;
	}
	{
		int best = -1;
		for (int i = 0; i < DEV_CACHE_SLOTS; i++)
			if (g_dev.p[i] && !g_dev.used[i] && g_dev.dev[i] == h->device && g_dev.cap[i] >= bytes &&
			    g_dev.cap[i] <= bytes + bytes / 2 + (1u << 20) && (best < 0 || g_dev.cap[i] < g_dev.cap[best]))
				best = i;
		if (best >= 0) {
			g_dev.used[best] = 1;
			g_dev.idle -= g_dev.cap[best];
			p = g_dev.p[best];
		}
	}
	pthread_mutex_unlock(&g_dev.mu);
	if (p)
		return p;
	if (hipMalloc(&p, bytes) != hipSuccess) {
		/* out of memory with idle buffers in the cache: give them back and try once more */
		pthread_mutex_lock(&g_dev.mu);
		for (int i = 0; i < DEV_CACHE_SLOTS; i++)
			if (g_dev.p[i] && !g_dev.used[i] && g_dev.dev[i] == h->device) {
				(void)hipFree(g_dev.p[i]);
				g_dev.idle -= g_dev.cap[i];
				g_dev.p[i] = NULL;
			}
		pthread_mutex_unlock(&g_dev.mu);
		if (hipMalloc(&p, bytes) != hipSuccess)
			return NULL;
	}
	pthread_mutex_lock(&g_dev.mu);
	for (int i = 0; i < DEV_CACHE_SLOTS && slot < 0; i++)
		if (!g_dev.p[i])
			slot = i;
	if (slot >= 0) { /* tracked: its size is known when it comes back (untracked ones are simply freed) */
		g_dev.p[slot] = p;
		g_dev.cap[slot] = bytes;
		g_dev.dev[slot] = h->device;
		g_dev.used[slot] = 1;
	}
	pthread_mutex_unlock(&g_dev.mu);
	return p;
}
static void dev_free(gpumt_ctx *h, void *p)
{
	int keep = 0, slot = -1;
	pthread_mutex_lock(&g_dev.mu);
	for (int i = 0; i < DEV_CACHE_SLOTS && slot < 0; i++)
		if (g_dev.p[i] == p && g_dev.used[i])
			slot = i;
	if (slot >= 0) {
		if (g_dev.idle + g_dev.cap[slot] <= g_dev.limit) {
			keep = 1;
			g_dev.idle += g_dev.cap[slot];
			g_dev.used[slot] = 0;
		} else {
			g_dev.p[slot] = NULL;
			g_dev.used[slot] = 0;
		}
	}
	pthread_mutex_unlock(&g_dev.mu);
	(void)h;
	if (!keep)
		(void)hipFree(p);
}

void *gpumt_malloc(gpumt_ctx *h, size_t bytes)
{
	if (!h || use(h))
		return NULL;
	return dev_alloc(h, bytes);
}
/* debug guard of the "free only idle buffers" contract (include/gpumt.h): a buffer handed back while any stream of its
 * context still has work queued is counted and reported, and the streams are drained before it is recycled */
static unsigned long g_free_busy;
static int free_guard(gpumt_ctx *h, const char *who, void *p)
{
	if (!h->debug_free)
		return 0;
	int busy = 0;
	for (int i = 0; i < GPUMT_NSTREAMS; i++)
		if (hipStreamQuery(h->st[i]) == hipErrorNotReady) {
			busy = 1;
			(void)hipStreamSynchronize(h->st[i]);
		}
	if (busy) {
		__atomic_fetch_add(&g_free_busy, 1ul, __ATOMIC_RELAXED);
		fprintf(stderr, "gpumt: %s(%p) with work queued on the context's streams (drained; GPUMT_DEBUG_FREE)\n", who, p);
	}
	return busy;
}
unsigned long gpumt_debug_free_busy(void) { return __atomic_exchange_n(&g_free_busy, 0ul, __ATOMIC_RELAXED); }

void gpumt_free(gpumt_ctx *h, void *p)
{
	/* the buffer must be idle: it may go to the cache and from there to another context without the
	 * device-wide wait hipFree implies */
	if (h && p && !use(h)) {
		(void)free_guard(h, "gpumt_free", p);
		dev_free(h, p);
	}
}
/*
 * Pinned host memory costs ~0.3 s per GiB to allocate and to free (page pinning), which used to be
 * most of a drop-in API call on a few GiB: freed staging buffers are therefore kept in a
 * process-wide cache and handed to the next context that asks (a decompress context after a
 * compress context, the next file of the CLI, the next call of a long-running caller).  The cache
 * is bounded (GPUMT_PINNED_CACHE_MB, default 16384); hipHostMallocPortable makes a buffer usable by
 * the contexts of every device.
 */
#define PIN_CACHE_SLOTS 64
static struct {
	pthread_mutex_t mu;
	void *p[PIN_CACHE_SLOTS];
	size_t cap[PIN_CACHE_SLOTS];
	size_t total, limit;
	int init;
} g_pin = {PTHREAD_MUTEX_INITIALIZER, {0}, {0}, 0, 0, 0};

struct pin_hdr { /* in front of every pinned buffer: its capacity */
	size_t cap;
	size_t pad[7];
};

void *gpumt_host_alloc(gpumt_ctx *h, size_t bytes)
{
	void *p = NULL;
	if (!h || use(h))
		return NULL;
	if (!bytes)
		bytes = 1;
	pthread_mutex_lock(&g_pin.mu);
	if (!g_pin.init) {
		const char *e = getenv("GPUMT_PINNED_CACHE_MB");
		g_pin.limit = (size_t)(e && *e ? strtoull(e, 0, 10) : 16384) << 20;
		g_pin.init = 1;
	}
	{
		int best = -1;
		for (int i = 0; i < PIN_CACHE_SLOTS; i++)
			if (g_pin.p[i] && g_pin.cap[i] >= bytes && g_pin.cap[i] <= bytes + bytes / 2 + (1u << 20) &&
			    (best < 0 || g_pin.cap[i] < g_pin.cap[best]))
				best = i;
		if (best >= 0) {
			p = g_pin.p[best];
			g_pin.total -= g_pin.cap[best];
			g_pin.p[best] = NULL;
		}
	}
	pthread_mutex_unlock(&g_pin.mu);
	if (p)
		return p;
	/* non-coherent = CPU-cached pinned memory: the callbacks memcpy in and out of it at full host
	 * speed; visibility is established by the stream synchronisation the engine does anyway */
	if (hipHostMalloc(&p, bytes + sizeof(struct pin_hdr), hipHostMallocNonCoherent | hipHostMallocPortable) !=
	    hipSuccess)
		return NULL;
	((struct pin_hdr *)p)->cap = bytes;
	return (u8 *)p + sizeof(struct pin_hdr);
}
void gpumt_host_free(gpumt_ctx *h, void *p)
{
	if (!h || !p)
		return;
	if (h->debug_free && !use(h))
		(void)free_guard(h, "gpumt_host_free", p);
	struct pin_hdr *hd = (struct pin_hdr *)((u8 *)p - sizeof(struct pin_hdr));
	const size_t cap = hd->cap;
	pthread_mutex_lock(&g_pin.mu);
	if (g_pin.total + cap <= g_pin.limit) {
		for (int i = 0; i < PIN_CACHE_SLOTS; i++)
			if (!g_pin.p[i]) {
				g_pin.p[i] = p;
				g_pin.cap[i] = cap;
				g_pin.total += cap;
				p = NULL;
				break;
			}
	}
	pthread_mutex_unlock(&g_pin.mu);
	if (p && !use(h))
		(void)hipHostFree(hd);
}

/* pin memory the caller owns (a mapping shared by the ranks of a multi-GPU job, an application buffer) so that
 * gpumt_memcpy_d2h / _h2d move it at copy-engine speed without a staging pass */
int gpumt_host_register(gpumt_ctx *h, void *p, size_t bytes)
{
	if (!h || !p || !bytes)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipHostRegister(p, bytes, hipHostRegisterPortable));
	return GPUMT_OK;
}
int gpumt_host_unregister(gpumt_ctx *h, void *p)
{
	if (!h || !p)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipHostUnregister(p));
	return GPUMT_OK;
}

/* give the idle buffers of the process-wide caches (device memory of this context's device, pinned host memory)
 * back to the system: a long-running host that compressed once does not have to keep up to 2 x 16 GiB alive.
 * Returns the number of bytes released. */
size_t gpumt_trim_caches(gpumt_ctx *h)
{
	size_t freed = 0;
	if (!h || use(h))
		return 0;
	pthread_mutex_lock(&g_dev.mu);
	for (int i = 0; i < DEV_CACHE_SLOTS; i++)
		if (g_dev.p[i] && !g_dev.used[i] && g_dev.dev[i] == h->device) {
			(void)hipFree(g_dev.p[i]);
			g_dev.idle -= g_dev.cap[i];
			freed += g_dev.cap[i];
			g_dev.p[i] = NULL;
		}
	pthread_mutex_unlock(&g_dev.mu);
	pthread_mutex_lock(&g_pin.mu);
	for (int i = 0; i < PIN_CACHE_SLOTS; i++)
		if (g_pin.p[i]) {
			(void)hipHostFree((u8 *)g_pin.p[i] - sizeof(struct pin_hdr));
			g_pin.total -= g_pin.cap[i];
			freed += g_pin.cap[i];
			g_pin.p[i] = NULL;
		}
	pthread_mutex_unlock(&g_pin.mu);
	return freed;
}

#define STREAM_OK(s) ((s) >= 0 && (s) < GPUMT_NSTREAMS)

int gpumt_memcpy_h2d(gpumt_ctx *h, void *dst, const void *src, size_t n, int s)
{
	if (!h || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, h->st[s]));
	return GPUMT_OK;
}
int gpumt_memcpy_d2h(gpumt_ctx *h, void *dst, const void *src, size_t n, int s)
{
	if (!h || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, h->st[s]));
	return GPUMT_OK;
}
int gpumt_push_host(gpumt_ctx *h, void *dst_host, const void *src, size_t n, const uint64_t *d_n, int s)
{
	void *dp = NULL;
	if (!h || !STREAM_OK(s) || ((uintptr_t)dst_host & 15) || ((uintptr_t)src & 15))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!n)
		return GPUMT_OK;
	CK(hipHostGetDevicePointer(&dp, dst_host, 0));
	const size_t nv = n >> 4;
	unsigned grid = (unsigned)((nv + 255) / 256);
	if (grid > 512)
		grid = 512; /* a few waves per CU saturate the host link and leave the rest to the codec kernels */
	if (grid < 1)
		grid = 1;
	hipLaunchKernelGGL(zmt_push_host_kernel, dim3(grid), dim3(256), 0, h->st[s], (const u8 *)src, (u8 *)dp, (u64)n,
			   (const u64 *)d_n);
	CK(hipGetLastError());
	return GPUMT_OK;
}
int gpumt_memcpy_d2d(gpumt_ctx *h, void *dst, const void *src, size_t n, int s)
{
	if (!h || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, h->st[s]));
	return GPUMT_OK;
}
int gpumt_memset(gpumt_ctx *h, void *dst, int byte, size_t n, int s)
{
	if (!h || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipMemsetAsync(dst, byte, n, h->st[s]));
	return GPUMT_OK;
}
int gpumt_stream_sync(gpumt_ctx *h, int s)
{
	if (!h || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipStreamSynchronize(h->st[s]));
	return GPUMT_OK;
}
int gpumt_device_sync(gpumt_ctx *h)
{
	if (!h)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipDeviceSynchronize());
	return GPUMT_OK;
}
int gpumt_mark(gpumt_ctx *h, int id, int s)
{
	if (!h || !STREAM_OK(s) || id < 0 || id >= GPUMT_NMARKS)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipEventRecord(h->mark[id], h->st[s]));
	return GPUMT_OK;
}
int gpumt_mark_sync(gpumt_ctx *h, int id)
{
	if (!h || id < 0 || id >= GPUMT_NMARKS)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipEventSynchronize(h->mark[id]));
	return GPUMT_OK;
}
int gpumt_stream_wait(gpumt_ctx *h, int waiter, int signaler)
{
	hipEvent_t ev;
	if (!h || !STREAM_OK(waiter) || !STREAM_OK(signaler))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* a fresh event per edge: edges may be in flight concurrently */
	CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	CK(hipEventRecord(ev, h->st[signaler]));
	CK(hipStreamWaitEvent(h->st[waiter], ev, 0));
	CK(hipEventDestroy(ev)); /* destruction is deferred until the event completes */
	return GPUMT_OK;
}
void *gpumt_stream_handle(gpumt_ctx *h, int s)
{
	return (h && STREAM_OK(s)) ? (void *)h->st[s] : NULL;
}

int gpumt_timer_start(gpumt_ctx *h, int slot, int s)
{
	if (!h || slot < 0 || slot >= NTIMERS || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipEventRecord(h->t0[slot], h->st[s]));
	return GPUMT_OK;
}
int gpumt_timer_stop(gpumt_ctx *h, int slot, int s)
{
	if (!h || slot < 0 || slot >= NTIMERS || !STREAM_OK(s))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipEventRecord(h->t1[slot], h->st[s]));
	return GPUMT_OK;
}
int gpumt_timer_ms(gpumt_ctx *h, int slot, float *ms)
{
	if (!h || slot < 0 || slot >= NTIMERS || !ms)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	CK(hipEventSynchronize(h->t1[slot]));
	CK(hipEventElapsedTime(ms, h->t0[slot], h->t1[slot]));
	return GPUMT_OK;
}

/* ------------------------------------------------------------------------------- LZ4 */
size_t gpumt_lz4_slot_stride(size_t chunk)
{
	size_t full = chunk / 65536, part = chunk % 65536;
	size_t b = 12 + 19 + 4 * (full + (part ? 1 : 0)) + chunk + 8;
	return (b + 255) & ~(size_t)255;
}

size_t gpumt_lz4_record_count(size_t n, size_t chunk)
{
	if (!chunk)
		return 0;
	return n ? (n + chunk - 1) / chunk : 1;
}

int gpumt_xxh32_batch(gpumt_ctx *h, const void *d_base, const uint64_t *d_off,
		      const uint32_t *d_len, size_t n, uint32_t *d_hash, int s)
{
	if (!h || !STREAM_OK(s) || n > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!n)
		return GPUMT_OK;
	hipLaunchKernelGGL(zmt_xxh32_kernel, dim3((unsigned)((n * 4 + 255) / 256)), dim3(256), 0,
			   h->st[s], (const u8 *)d_base, d_off, d_len, (u32)n, d_hash,
			   (const u32 *)NULL, (const u32 *)NULL, (u32 *)NULL);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk,
			     void *d_slots, size_t slot_stride, uint32_t *d_rec_len, int s)
{
	return gpumt_lz4_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, 1, s);
}

int gpumt_lz4_level_supported(int level) { return level >= 1 && level <= 12; }

int gpumt_lz4_compress_batch_level(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk,
				   void *d_slots, size_t slot_stride, uint32_t *d_rec_len, int level, int s)
{
	size_t nrec = gpumt_lz4_record_count(n, chunk);
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > 0x40000000u || nrec > 0x3FFFFFFFu ||
	    slot_stride < gpumt_lz4_slot_stride(chunk) || !gpumt_lz4_level_supported(level))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* scratch: off[nrec] u64 | len[nrec] u32 | chk[nrec] u32 | (HC) one table set per wave */
	const bool hc = level >= 3;
	const size_t hc_max = h->hc_waves > 0 ? (size_t)h->hc_waves : GPUMT_LZ4HC_WAVES;
	const size_t hc_grid = nrec < hc_max ? nrec : hc_max;
	const size_t hc_base = (nrec * 16 + 255) & ~(size_t)255;
	if (want_scratch(h, 0, s, hc ? hc_base + hc_grid * GPUMT_LZ4HC_SCRATCH : nrec * 16))
		return GPUMT_E_HIP;
	u64 *off = (u64 *)h->scratch[0][s];
	u32 *len = (u32 *)(off + nrec);
	u32 *chk = len + nrec;
	hipLaunchKernelGGL(zmt_iota_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0,
			   h->st[s], off, len, (u64)n, (u64)chunk, (u32)nrec);
	PROF0(8);
	hipLaunchKernelGGL(zmt_xxh32_kernel, dim3((unsigned)((nrec * 4 + 255) / 256)), dim3(256), 0,
			   h->st[s], (const u8 *)d_in, (const u64 *)off, (const u32 *)len, (u32)nrec,
			   chk, (const u32 *)NULL, (const u32 *)NULL, (u32 *)NULL);
	PROF1(8);
	PROF0(9);
	unsigned long long *eprof = NULL;
	if (h->profile == 4) {
		if (!h->d_prof) {
			CK(hipMalloc((void **)&h->d_prof, 16 * sizeof(unsigned long long)));
			CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
		}
		eprof = h->d_prof;
	}
	if (hc) {
		/* levels 3..9: hash-chain parser, 10..12: optimal parser (lz4_enc_hc.hip) */
		hipLaunchKernelGGL(zmt_lz4hc_enc_kernel, dim3((unsigned)hc_grid), dim3(64), 0, h->st[s],
				   (const u8 *)d_in, (u64)n, (u32)chunk, (u32)nrec, (u8 *)d_slots,
				   (u64)slot_stride, d_rec_len, (const u32 *)chk,
				   (u8 *)h->scratch[0][s] + hc_base, level);
	} else {
		/* chunk <= 64 KiB: every record is a single independent block (byU16 table).  Else linked-block records
		 * (17-bit entries up to 128 KiB chunks, 32-bit beyond); the ragged last record may be <= 64 KiB and then
		 * belongs to the byU16 kernel (each kernel skips records of the other kind) */
		const bool v3 = h->enc_variant == 3 || eprof;
		typedef void (*enc_fn)(const u8 *, u64, u32, u32, u32, u8 *, u64, u32 *, const u32 *, unsigned long long *);
		const enc_fn k16 = v3 ? zmt_lz4_enc3_u16_kernel : zmt_lz4_enc5_u16_kernel;
		const enc_fn k17 = eprof ? zmt_lz4_enc3_p17_prof_kernel : v3 ? zmt_lz4_enc3_p17_kernel : zmt_lz4_enc5_p17_kernel;
		const enc_fn k32 = v3 ? zmt_lz4_enc3_u32_kernel : zmt_lz4_enc5_u32_kernel;
		if (chunk <= 65536) {
			hipLaunchKernelGGL(k16, dim3((unsigned)nrec), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
					   (u32)chunk, 0u, (u32)nrec, (u8 *)d_slots, (u64)slot_stride, d_rec_len,
					   (const u32 *)chk, eprof);
		} else {
			hipLaunchKernelGGL(chunk <= 131072 ? k17 : k32, dim3((unsigned)nrec), dim3(64),
					   chunk <= 131072 ? (size_t)h->xflags : 0 /* developer: dynamic-LDS padding = occupancy knob */,
					   h->st[s], (const u8 *)d_in, (u64)n, (u32)chunk, 0u, (u32)nrec, (u8 *)d_slots,
					   (u64)slot_stride, d_rec_len, (const u32 *)chk, eprof);
			hipLaunchKernelGGL(k16, dim3(1), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n, (u32)chunk,
					   (u32)(nrec - 1), (u32)nrec, (u8 *)d_slots, (u64)slot_stride, d_rec_len,
					   (const u32 *)chk, (unsigned long long *)NULL);
		}
	}
	PROF1(9);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_compact(gpumt_ctx *h, const void *d_slots, size_t slot_stride,
		      const uint32_t *d_rec_len, size_t nrec, void *d_stream, uint64_t *d_rec_off,
		      int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	PROF0(10);
	hipLaunchKernelGGL(zmt_scan_kernel, dim3(1), dim3(1024), 0, h->st[s], d_rec_len, (u32)nrec,
			   d_rec_off);
	hipLaunchKernelGGL(zmt_compact_kernel, dim3((unsigned)nrec), dim3(256), 0, h->st[s],
			   (const u8 *)d_slots, (u64)slot_stride, d_rec_len,
			   (const u64 *)d_rec_off, (u32)nrec, (u8 *)d_stream);
	PROF1(10);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_probe_sizes(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
			  const uint32_t *d_rec_len, size_t nrec, uint32_t *d_out_len,
			  uint64_t *d_out_off, int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	hipLaunchKernelGGL(zmt_probe_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0,
			   h->st[s], (const u8 *)d_stream, d_rec_off, d_rec_len, (u32)nrec,
			   d_out_len);
	hipLaunchKernelGGL(zmt_scan_kernel, dim3(1), dim3(1024), 0, h->st[s],
			   (const u32 *)d_out_len, (u32)nrec, d_out_off);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* The record decoders.  gpumt_lz4_decompress_batch passes no kept array and no checksum words: it launches the kernels it
 * always launched, the words lie in the scratch and the verify pass follows.  gpumt_lz4_decompress_batch_par passes its
 * scratch status words as `kept` (ST_REC_KEPT = the block stages decoded the record) and checksum words of its own: the frame
 * and the serial kernel are then their _kept entries -- the frame kernel leaves such a record's block-table slots empty and
 * writes that word to d_status, so parse4, copy3 and the serial kernel pass it by -- and the verify pass is the caller's. */
static int lz4_decompress_records(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				  const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				  const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, const u32 *kept, u32 *x_ce,
				  u32 *x_cv, int s)
{
	const u32 n = (u32)nrec;
	const unsigned g256 = (unsigned)((nrec + 255) / 256);
	/* scratch carve-up (all offsets 16-byte aligned) */
	const size_t nblk_max = out_bytes / 65536 + nrec + 1;
	const size_t ntok_max = stream_bytes / 3 + 128 * nblk_max + 256;
	size_t off = 0;
#define CARVE(var, type, count)                                                                    \
	size_t var##_o = off;                                                                      \
	off += (((size_t)(count) * sizeof(type)) + 15) & ~(size_t)15;
	CARVE(ce, u32, nrec)
	CARVE(cv, u32, nrec)
	CARVE(est, u32, nrec)
	CARVE(blk0, u64, nrec + 1)
	CARVE(rnb, u32, nrec)
	CARVE(rfl, u32, nrec)
	CARVE(bco, u64, nblk_max)
	CARVE(bcs, u32, nblk_max)
	CARVE(bnt, u32, nblk_max)
	CARVE(bol, u32, nblk_max)
	CARVE(tok, u16, ntok_max)
#undef CARVE
	const bool split = h->dec_variant == 0;
	if (h->profile >= 2 && !h->d_prof) {
		CK(hipMalloc((void **)&h->d_prof, 16 * sizeof(unsigned long long)));
		CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
	}
	if (want_scratch(h, 1, s, split ? off : nrec * 8 + 32))
		return GPUMT_E_HIP;
	u8 *sc = (u8 *)h->scratch[1][s];
	u32 *ce = x_ce ? x_ce : (u32 *)(sc + ce_o), *cv = x_ce ? x_cv : (u32 *)(sc + cv_o);
	PROF0(11);
	if (split) {
		u32 *est = (u32 *)(sc + est_o), *rnb = (u32 *)(sc + rnb_o), *rfl = (u32 *)(sc + rfl_o);
		u64 *blk0 = (u64 *)(sc + blk0_o), *bco = (u64 *)(sc + bco_o);
		u32 *bcs = (u32 *)(sc + bcs_o), *bnt = (u32 *)(sc + bnt_o), *bol = (u32 *)(sc + bol_o);
		u16 *tok = (u16 *)(sc + tok_o);
		PROF0(13);
		hipLaunchKernelGGL(zmt_dec_nblk_kernel, dim3(g256), dim3(256), 0, h->st[s], d_out_len, n, est);
		hipLaunchKernelGGL(zmt_scan_kernel, dim3(1), dim3(1024), 0, h->st[s], (const u32 *)est, n, blk0);
		if (kept)
			hipLaunchKernelGGL(zmt_dec_frames_kept_kernel, dim3(g256), dim3(256), 0, h->st[s],
					   (const u8 *)d_stream, d_rec_off, d_rec_len, n, d_out_len,
					   (const u64 *)blk0, bco, bcs, rnb, rfl, d_status, ce, cv, kept);
		else
			hipLaunchKernelGGL(zmt_dec_frames_kernel, dim3(g256), dim3(256), 0, h->st[s],
					   (const u8 *)d_stream, d_rec_off, d_rec_len, n, d_out_len,
					   (const u64 *)blk0, bco, bcs, rnb, rfl, d_status, ce, cv);
		PROF1(13);
		const int ring = h->lz4_ring < 12 ? 12 : h->lz4_ring > 14 ? 14 : h->lz4_ring;
		PROF0(14);
		hipLaunchKernelGGL(zmt_dec_parse4_kernel, dim3((unsigned)((nblk_max + 63) / 64)), dim3(64), 0,
				   h->st[s], (const u8 *)d_stream, (u64)stream_bytes, (const u64 *)bco,
				   (const u32 *)bcs, (const u64 *)(blk0 + nrec), tok, bnt, bol);
		PROF1(14);
		PROF0(15);
#define C3_LAUNCH(NAME)                                                                                            \
	hipLaunchKernelGGL(NAME, dim3((unsigned)nrec), dim3(64), (size_t)h->dec_pad, h->st[s], (const u8 *)d_stream, \
			   (u64)stream_bytes, 0u, n, (u8 *)d_out, d_out_off, d_out_len, (const u64 *)blk0,         \
			   (const u64 *)bco, (const u32 *)bcs, (const u32 *)rnb, (const u32 *)rfl, (const u16 *)tok, \
			   (const u32 *)bnt, (const u32 *)bol, d_status)
#define C3_LAUNCHP(NAME)                                                                                           \
	hipLaunchKernelGGL(NAME, dim3((unsigned)nrec), dim3(64), 0, h->st[s], (const u8 *)d_stream,               \
			   (u64)stream_bytes, 0u, n, (u8 *)d_out, d_out_off, d_out_len, (const u64 *)blk0,         \
			   (const u64 *)bco, (const u32 *)bcs, (const u32 *)rnb, (const u32 *)rfl, (const u16 *)tok, \
			   (const u32 *)bnt, (const u32 *)bol, d_status, h->d_prof)
		/* (one stream, one launch per stage.  Slices of the records on internal streams -- a slice's parse under the copy of
		 * the one before it, its XXH32 verify under the copy of the next -- were built and measured in rounds 2 and 6: a kernel
		 * that arrives while the device is full of copy waves is starved, not interleaved, and a slice's parse lasts as long as
		 * the whole batch's; 13.4-32.9 ms against 13.55, profiles/r06_sweeps/lz4_dec_slices.txt) */
		if (h->profile == 8) {
			if (ring == 12)
				C3_LAUNCHP(zmt_dec_copy3_w4_kernel_prof);
			else if (ring == 13)
				C3_LAUNCHP(zmt_dec_copy3_w8_kernel_prof);
			else
				C3_LAUNCHP(zmt_dec_copy3_w16_kernel_prof);
		} else {
			if (ring == 12)
				C3_LAUNCH(zmt_dec_copy3_w4_kernel);
			else if (ring == 13)
				C3_LAUNCH(zmt_dec_copy3_w8_kernel);
			else
				C3_LAUNCH(zmt_dec_copy3_w16_kernel);
		}
		PROF1(15);
		/* records the fast path does not cover (block size > 64 KiB, odd block counts) */
		if (kept)
			hipLaunchKernelGGL(zmt_lz4_dec_serial_kept, dim3(n), dim3(64), 0, h->st[s], (const u8 *)d_stream,
					   d_rec_off, d_rec_len, n, (u8 *)d_out, d_out_off, d_out_len, d_status, ce,
					   cv, 100u, kept);
		else
			hipLaunchKernelGGL(zmt_lz4_dec_serial, dim3(n), dim3(64), 0, h->st[s], (const u8 *)d_stream,
					   d_rec_off, d_rec_len, n, (u8 *)d_out, d_out_off, d_out_len, d_status, ce,
					   cv, 100u);
	} else if (kept) {
		hipLaunchKernelGGL(zmt_lz4_dec_serial_kept, dim3(n), dim3(64), 0, h->st[s], (const u8 *)d_stream,
				   d_rec_off, d_rec_len, n, (u8 *)d_out, d_out_off, d_out_len, d_status, ce,
				   cv, 0xFFFFFFFFu, kept);
	} else {
		hipLaunchKernelGGL(zmt_lz4_dec_serial, dim3(n), dim3(64), 0, h->st[s], (const u8 *)d_stream,
				   d_rec_off, d_rec_len, n, (u8 *)d_out, d_out_off, d_out_len, d_status, ce,
				   cv, 0xFFFFFFFFu);
	}
	PROF1(11);
	if (!x_ce) {
		PROF0(12);
		hipLaunchKernelGGL(zmt_xxh32_kernel, dim3((unsigned)((nrec * 4 + 255) / 256)), dim3(256), 0,
				   h->st[s], (const u8 *)d_out, d_out_off, d_out_len, n, (u32 *)NULL,
				   (const u32 *)ce, (const u32 *)cv, d_status);
		PROF1(12);
	}
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_decompress_batch(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
			       const uint64_t *d_rec_off, const uint32_t *d_rec_len, size_t nrec,
			       void *d_out, size_t out_bytes, const uint64_t *d_out_off,
			       uint32_t *d_out_len, uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	return lz4_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off, d_out_len,
				      d_status, NULL, NULL, NULL, s);
}

int gpumt_lz4_decompress_blocks(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				const gpumt_lz4_block *d_blocks, size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun,
				void *d_out, size_t out_bytes, uint32_t *d_block_len, uint32_t *d_run_len,
				uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || !d_stream || !d_blocks || !d_runs || !d_out || !d_block_len || !d_run_len || !d_status ||
	    nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	PROF0(11);
	hipLaunchKernelGGL(zmt_lz4_dec_blocks_kernel, dim3((unsigned)nrun), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out, (u64)out_bytes,
			   d_block_len, d_run_len, d_status);
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_decompress_blocks_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				    const gpumt_lz4_block *d_blocks, size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun,
				    void *d_out, size_t out_bytes, uint32_t *d_block_len, uint32_t *d_run_len,
				    uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || !d_stream || !d_blocks || !d_runs || !d_out || !d_block_len || !d_run_len || !d_status ||
	    nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* the origin plane (one u16 per byte of d_out) + five words per block + the plan's flag */
	const size_t plane = (GPUMT_LZ4_PAR_SCRATCH(out_bytes) + 255) & ~(size_t)255;
	const size_t need = (plane + nblk * 20 + 256 + 0xFFFFF) & ~(size_t)0xFFFFF;
	/* a table without a run of two blocks (every frame of independent blocks) has nothing to decode side by side */
	int par = h->lrun_par != 0 && nblk > nrun && !(h->lrun_par_refused && need >= h->lrun_par_refused);
	if (par && need > h->scratch_bytes[1][s]) {
		/* as gpumt_zstd_decompress_blocks_pre: the larger area first, a refused size is not asked for again */
		void *p = dev_alloc(h, need);
		if (!p) {
			(void)hipGetLastError(); /* (a refused allocation is no error of this call) */
			h->lrun_par_refused = need;
			par = 0;
		} else {
			if (h->scratch[1][s]) {
				if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
					dev_free(h, p);
					return GPUMT_E_HIP;
				}
				dev_free(h, h->scratch[1][s]);
			}
			h->scratch[1][s] = p;
			h->scratch_bytes[1][s] = need;
		}
	}
	if (!par)
		return gpumt_lz4_decompress_blocks(h, d_stream, stream_bytes, d_blocks, nblk, d_runs, nrun, d_out, out_bytes,
						   d_block_len, d_run_len, d_status, s);
	Lz4Par P;
	P.origin = (u16 *)h->scratch[1][s];
	P.owner = (u32 *)((u8 *)h->scratch[1][s] + plane);
	P.mlen = P.owner + nblk;
	P.mst = P.mlen + nblk;
	P.pos = P.mst + nblk;
	P.xst = P.pos + nblk;
	P.flag = P.xst + nblk;
	PROF0(11);
	CK(hipMemsetAsync(P.owner, 0xFF, nblk * 4, h->st[s]));
	CK(hipMemsetAsync(P.flag, 0, 4, h->st[s]));
	hipLaunchKernelGGL(zmt_lz4_par_plan_kernel, dim3(1), dim3(64), 0, h->st[s], d_runs, (u32)nrun, (u32)nblk, (u64)out_bytes, P);
	hipLaunchKernelGGL(zmt_lz4_par_measure_kernel, dim3((unsigned)nblk), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, P);
	hipLaunchKernelGGL(zmt_lz4_par_scan_kernel, dim3((unsigned)nrun), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out, (u64)out_bytes, d_block_len,
			   d_run_len, d_status, P);
	hipLaunchKernelGGL(zmt_lz4_par_exec_kernel, dim3((unsigned)nblk), dim3(64), 0, h->st[s], (const u8 *)d_stream, d_blocks,
			   (u32)nblk, d_runs, (u8 *)d_out, P);
	hipLaunchKernelGGL(zmt_lz4_par_resolve_kernel, dim3((unsigned)nrun), dim3(1024), 0, h->st[s], d_runs, (u32)nrun,
			   (u32)nblk, (u8 *)d_out, (u64)out_bytes, d_block_len, d_run_len, d_status, P);
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_decompress_blocks_seg(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				    const gpumt_lz4_block *d_blocks, size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun,
				    void *d_out, size_t out_bytes, uint32_t *d_block_len, uint32_t *d_run_len,
				    uint32_t *d_status, uint32_t *d_block_seg, int s)
{
	if (!h || !STREAM_OK(s) || !d_stream || !d_blocks || !d_runs || !d_out || !d_block_len || !d_run_len || !d_status ||
	    !d_block_seg || nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* the origin plane, then the cuts (two words each), one word per slot, six words per block + the plan's flag */
	const size_t seg = (size_t)h->lseg_bytes, ncut = out_bytes / seg + nblk;
	const size_t plane = (GPUMT_LZ4_PAR_SCRATCH(out_bytes) + 255) & ~(size_t)255;
	const size_t need = (GPUMT_LZ4_SEG_SCRATCH(out_bytes, nblk, seg) + 512 + 0xFFFFF) & ~(size_t)0xFFFFF;
	int par = h->lblk_seg != 0 && nblk != 0 && ncut + nblk <= 0x7FFFFFFFu &&
		  !(h->lblk_seg_refused && need >= h->lblk_seg_refused);
	if (nblk)
		CK(hipMemsetAsync(d_block_seg, 0, nblk * 4, h->st[s]));
	if (par && need > h->scratch_bytes[1][s]) {
		/* as gpumt_lz4_decompress_blocks_par, whose cached area this is */
		void *p = dev_alloc(h, need);
		if (!p) {
			(void)hipGetLastError(); /* (a refused allocation is no error of this call) */
			h->lblk_seg_refused = need;
			par = 0;
		} else {
			if (h->scratch[1][s]) {
				if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
					dev_free(h, p);
					return GPUMT_E_HIP;
				}
				dev_free(h, h->scratch[1][s]);
			}
			h->scratch[1][s] = p;
			h->scratch_bytes[1][s] = need;
		}
	}
	if (!par)
		return gpumt_lz4_decompress_blocks(h, d_stream, stream_bytes, d_blocks, nblk, d_runs, nrun, d_out, out_bytes,
						   d_block_len, d_run_len, d_status, s);
	Lz4Seg P;
	P.origin = (u16 *)h->scratch[1][s];
	P.cut = (u32 *)((u8 *)h->scratch[1][s] + plane);
	P.xst = P.cut + 2 * ncut;
	P.owner = P.xst + ncut + nblk;
	P.mlen = P.owner + nblk;
	P.mst = P.mlen + nblk;
	P.pos = P.mst + nblk;
	P.nseg = P.pos + nblk;
	P.cbase = P.nseg + nblk;
	P.flag = P.cbase + nblk + 1;
	P.shift = (u32)__builtin_ctzl(seg);
	P.ncut = (u32)ncut;
	PROF0(11);
	CK(hipMemsetAsync(P.owner, 0xFF, nblk * 4, h->st[s]));
	CK(hipMemsetAsync(P.flag, 0, 4, h->st[s]));
	hipLaunchKernelGGL(zmt_lz4_seg_plan_kernel, dim3(1), dim3(64), 0, h->st[s], d_blocks, (u32)nblk, d_runs, (u32)nrun,
			   (u64)out_bytes, P);
	hipLaunchKernelGGL(zmt_lz4_seg_measure_kernel, dim3((unsigned)nblk), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, P);
	hipLaunchKernelGGL(zmt_lz4_seg_scan_kernel, dim3((unsigned)nrun), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out, (u64)out_bytes, d_block_len,
			   d_run_len, d_status, P);
	hipLaunchKernelGGL(zmt_lz4_seg_exec_kernel, dim3((unsigned)(ncut + nblk)), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   d_blocks, (u32)nblk, d_runs, (u8 *)d_out, P);
	hipLaunchKernelGGL(zmt_lz4_seg_resolve_kernel, dim3((unsigned)nrun), dim3(1024), 0, h->st[s], d_runs, (u32)nrun,
			   (u32)nblk, (u8 *)d_out, (u64)out_bytes, d_block_len, d_run_len, d_status, d_block_seg, P);
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_lz4_pack_runs(gpumt_ctx *h, const void *d_out, size_t out_bytes, const gpumt_lz4_run *d_runs,
			const uint32_t *d_run_len, size_t nrun, void *d_packed, size_t packed_bytes,
			uint64_t *d_pack_off, int s)
{
	if (!h || !STREAM_OK(s) || !d_out || !d_runs || !d_run_len || !d_packed || !d_pack_off || nrun == 0 ||
	    nrun > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	/* the two areas must not overlap: the runs are moved side by side */
	if ((const u8 *)d_packed < (const u8 *)d_out + out_bytes && (const u8 *)d_out < (const u8 *)d_packed + packed_bytes)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	PROF0(10);
	hipLaunchKernelGGL(zmt_scan_kernel, dim3(1), dim3(1024), 0, h->st[s], d_run_len, (u32)nrun, d_pack_off);
	hipLaunchKernelGGL(zmt_lz4_gather_runs_kernel, dim3((unsigned)nrun), dim3(256), 0, h->st[s], (const u8 *)d_out,
			   (u64)out_bytes, d_runs, d_run_len, (const u64 *)d_pack_off, (u32)nrun, (u8 *)d_packed,
			   (u64)packed_bytes);
	PROF1(10);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_xxh32_carry(gpumt_ctx *h, const void *d_base, size_t base_bytes, const gpumt_xxh32_job *d_jobs, size_t njobs,
		      uint32_t *d_states, uint32_t *d_digest, uint32_t *d_verdict, int s)
{
	if (!h || !STREAM_OK(s) || !d_base || !d_jobs || !d_states || !d_digest || !d_verdict || njobs > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!njobs)
		return GPUMT_OK;
	PROF0(12);
	hipLaunchKernelGGL(zmt_xxh32_carry_kernel, dim3((unsigned)njobs), dim3(64), 0, h->st[s], (const u8 *)d_base,
			   (u64)base_bytes, d_jobs, (u32)njobs, d_states, d_digest, d_verdict);
	PROF1(12);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* ------------------------------------------------------------------ zstd */
#define ZE_BLOCK 131072u
#define ZE_BSTRIDE (ZE_BLOCK + 16u)
#define ZE_HDR 32u
#define ZE_MAXSEQ (ZE_BLOCK / 4u)
#define ZE_WSCRATCH_BYTES ((size_t)3 * ZE_MAXSEQ * 4 + 16 * 20544 + ZE_BLOCK + 64) /* per persistent encoder wave (zstd_enc.hip) */

size_t gpumt_zstd_slot_stride(size_t chunk)
{
	const size_t nb = chunk ? (chunk + ZE_BLOCK - 1) / ZE_BLOCK : 1;
	return (ZE_HDR + nb * ZE_BSTRIDE + 255) & ~(size_t)255;
}

/* level -> encoder tier (zstd_enc.hip): 1-2 the fast parse (4 Ki-entry table, 16 waves per CU), 3-9 and 10-22
 * larger tables and a 6-byte hash (8 / 4 waves per CU) */
int gpumt_zstd_level_tier(int level) { return level <= 2 ? 0 : level <= 9 ? 1 : 2; }

int gpumt_zstd_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
			      size_t slot_stride, uint32_t *d_rec_len, int s)
{
	return gpumt_zstd_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, 1, s);
}

int gpumt_zstd_compress_batch_level(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				    size_t slot_stride, uint32_t *d_rec_len, int level, int s)
{
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > 0x40000000u || slot_stride < gpumt_zstd_slot_stride(chunk) ||
	    level < 1 || level > 22)
		return GPUMT_E_ARG;
	const int tier = h->profile == 6 ? 0 : gpumt_zstd_level_tier(level);
	if (use(h))
		return GPUMT_E_HIP;
	const size_t nrec = gpumt_lz4_record_count(n, chunk);
	const u32 bpr = (u32)((chunk + ZE_BLOCK - 1) / ZE_BLOCK);
	const size_t nblk = nrec * bpr;
	if (nblk > 0x7FFFFFFFu)
		return GPUMT_E_ARG;
	/* persistent waves, exactly as many as stay resident (LDS-limited), blocks taken round-robin */
	if (!h->zenc_waves[tier]) {
		int per_cu = 0;
		if (tier == 0)
			CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_zstd_enc_kernel, 64, 0));
		else if (tier == 1)
			CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_zstd_enc_t2_kernel, 64, 0));
		else
			CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_zstd_enc_t3_kernel, 64, 0));
		h->zenc_waves[tier] = (per_cu > 0 ? per_cu : 4) * (h->num_cus > 0 ? h->num_cus : 256);
	}
	const unsigned grid = (unsigned)(nblk < (size_t)h->zenc_waves[tier] ? nblk : (size_t)h->zenc_waves[tier]);
	const size_t seq_bytes = (size_t)grid * (3 * ZE_MAXSEQ * 4 + 16 * 20544 + ZE_BLOCK + 64);
	if (h->profile == 6)
		fprintf(stderr, "gpumt: zstd encoder grid %u waves\n", grid);
	if (want_scratch(h, 0, s, nblk * 4 + 64 + seq_bytes))
		return GPUMT_E_HIP;
	u32 *blk_len = (u32 *)h->scratch[0][s];
	u8 *seqbuf = (u8 *)h->scratch[0][s] + ((nblk * 4 + 63) & ~(size_t)63);
	if (h->profile == 6 && !h->d_prof) {
		CK(hipMalloc((void **)&h->d_prof, 16 * sizeof(unsigned long long)));
		CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
	}
	PROF0(9);
	if (h->profile == 6)
		hipLaunchKernelGGL(zmt_zstd_enc_kernel_prof, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in,
				   (u64)n, (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len,
				   seqbuf, h->d_prof);
	else if (tier == 0)
		hipLaunchKernelGGL(zmt_zstd_enc_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
				   (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len, seqbuf);
	else if (tier == 1)
		hipLaunchKernelGGL(zmt_zstd_enc_t2_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
				   (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len, seqbuf);
	else
		hipLaunchKernelGGL(zmt_zstd_enc_t3_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
				   (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len, seqbuf);
	hipLaunchKernelGGL(zmt_zstd_assemble_kernel, dim3((unsigned)nrec), dim3(256), 0, h->st[s], (u64)n,
			   (u32)chunk, (u32)nrec, bpr, (u8 *)d_slots, (u64)slot_stride, (const u32 *)blk_len,
			   d_rec_len);
	PROF1(9);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* ---- the whole chunk as the match window (zstd_enc_win.h) ---- */
#define ZW_HLOG_MAX 17
#define ZW_HLOG_MIN 12
#define ZW_MAXDIST (1u << 27)
#define ZW_SLICE ((size_t)1 << 30) /* input bytes per launch slice: the plane stays within 4 GiB */

/* ---- its chain plane, for the brotli encoder's window as well: one wave per chunk (zmt_zstd_win_chain_kernel) or, with
 * "win_chain_par", in segments (enc_win_chain_par.h) ---- */
#define GPUMT_WIN_CHAIN_SEG_DEFAULT 20 /* the lowest median at level 10 and 8 MiB chunks: profiles/win_chain_par.txt */

static u32 zw_hlog_host(size_t clen) /* zw_hlog of zstd_enc_win.h */
{
	const int l = 63 - __builtin_clzll((unsigned long long)clen | 1ull) - 3;
	return (u32)(l > ZW_HLOG_MAX ? ZW_HLOG_MAX : l < ZW_HLOG_MIN ? ZW_HLOG_MIN : l);
}

size_t gpumt_win_chain_par_scratch(size_t n, size_t chunk, int seg_log)
{
	if (!n || !chunk || seg_log < 12 || seg_log > 24)
		return 0;
	const size_t cl = n < chunk ? n : chunk, spc = (cl + ((size_t)1 << seg_log) - 1) >> seg_log;
	if (spc <= 1)
		return 0; /* no chunk has more than one segment: the serial kernel builds the plane */
	return ((n + chunk - 1) / chunk * spc * 4) << zw_hlog_host(cl);
}

static int wchain_seg_log(const gpumt_ctx *h) { return h->wchain_par == 1 ? GPUMT_WIN_CHAIN_SEG_DEFAULT : h->wchain_par; }

/* scratch[0][s] grown to `need` bytes, asked for before the area the stream has is let go: 1 = it holds them, 0 = the
 * device refused and the old area stays, < 0 = an error */
static int win_scratch_grow(gpumt_ctx *h, size_t need, int s)
{
	if (need <= h->scratch_bytes[0][s])
		return 1;
	void *p = dev_alloc(h, need);
	if (!p) {
		(void)hipGetLastError(); /* (a refused allocation is no error of the call) */
		return 0;
	}
	if (h->scratch[0][s]) {
		if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
			dev_free(h, p);
			return GPUMT_E_HIP;
		}
		dev_free(h, h->scratch[0][s]);
	}
	h->scratch[0][s] = p;
	h->scratch_bytes[0][s] = need;
	return 1;
}

/* the _win calls with "win_chain_par" on ask for their scratch and `pheads` bytes of head tables behind it, `total`
 * together, first: 1 = granted, 0 = refused -- by "win_chain_cap_mb", by the call's own cap (own_cap_mb), by the device, or
 * because the device refused that much before -- and the serial kernel builds the plane; < 0 = an error */
static int win_chain_par_ask(gpumt_ctx *h, size_t total, size_t pheads, int own_cap_mb, int s)
{
	if (h->wchain_refused && pheads >= h->wchain_refused)
		return 0;
	if (h->wchain_cap_mb && pheads > ((size_t)h->wchain_cap_mb << 20)) {
		h->wchain_refused = pheads;
		return 0;
	}
	if (own_cap_mb && total > ((size_t)own_cap_mb << 20))
		return 0;
	const int r = win_scratch_grow(h, total, s);
	if (r == 0)
		h->wchain_refused = pheads;
	return r;
}

/* the plane of one slice (nr records, ni bytes) on stream s.  heads = a table of 4 << ZW_HLOG_MAX bytes per wave of the
 * serial kernel's grid cg; pheads = gpumt_win_chain_par_scratch(ni, chunk, seg_log) bytes or NULL.  With pheads and a chunk of
 * more than one segment: the three launches of enc_win_chain_par.h; else the serial kernel, as before */
static int win_chain_launch(gpumt_ctx *h, const u8 *in, size_t ni, size_t chunk, size_t nr, u32 *plane, u32 *heads, unsigned cg,
			    u32 *pheads, int seg_log, int s)
{
	if (!pheads || !gpumt_win_chain_par_scratch(ni, chunk, seg_log)) {
		hipLaunchKernelGGL(zmt_zstd_win_chain_kernel, dim3(cg), dim3(64), 0, h->st[s], in, (u64)ni, (u32)chunk, (u32)nr, plane,
				   heads);
		return GPUMT_OK;
	}
	if (!h->wchain_waves) {
		int per_cu = 0;
		CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_win_chain_seg_kernel, 64, 0));
		h->wchain_waves = (per_cu > 0 ? per_cu : 4) * (h->num_cus > 0 ? h->num_cus : 256);
	}
	const size_t cl = ni < chunk ? ni : chunk, spc = (cl + ((size_t)1 << seg_log) - 1) >> seg_log, nseg = nr * spc;
	const u32 hslog = zw_hlog_host(cl);
	const unsigned sg = (unsigned)(nseg < (size_t)h->wchain_waves ? nseg : (size_t)h->wchain_waves);
	hipLaunchKernelGGL(zmt_win_chain_seg_kernel, dim3(sg), dim3(64), 0, h->st[s], in, (u64)ni, (u32)chunk, (u32)seg_log,
			   (u32)spc, (u32)nseg, hslog, plane, pheads);
	hipLaunchKernelGGL(zmt_win_chain_carry_kernel, dim3((unsigned)((nr << hslog) / 256)), dim3(256), 0, h->st[s], (u64)ni,
			   (u32)chunk, (u32)seg_log, (u32)spc, (u32)nr, hslog, pheads);
	hipLaunchKernelGGL(zmt_win_chain_patch_kernel, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, h->st[s], in, (u64)ni,
			   (u32)chunk, (u32)seg_log, (u32)spc, hslog, plane, (const u32 *)pheads);
	return GPUMT_OK;
}

int gpumt_win_chain_plane(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, uint32_t *d_plane, int seg_log, int s)
{
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > ZW_MAXDIST || n > ZW_SLICE || (seg_log != 0 && (seg_log < 12 || seg_log > 24)) ||
	    (n && (!d_in || !d_plane)))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!n)
		return GPUMT_OK;
	const size_t nrec = gpumt_lz4_record_count(n, chunk);
	const size_t cwaves = (size_t)4 * (h->num_cus > 0 ? h->num_cus : 256), cgrid = nrec < cwaves ? nrec : cwaves;
	const size_t o_pheads = cgrid * 4 << ZW_HLOG_MAX, pheads = gpumt_win_chain_par_scratch(n, chunk, seg_log);
	const size_t need = (o_pheads + pheads + 0xFFFFF) & ~(size_t)0xFFFFF;
	/* this call never builds the plane another way than asked: refused head tables are an error */
	if ((pheads && h->wchain_cap_mb && pheads > ((size_t)h->wchain_cap_mb << 20)) || !win_scratch_grow(h, need, s)) {
		snprintf(h->err, sizeof h->err, "chain plane: %zu bytes of head tables refused", pheads ? pheads : o_pheads);
		return GPUMT_E_NOMEM;
	}
	if (need > h->scratch_bytes[0][s])
		return GPUMT_E_HIP; /* (win_scratch_grow: the stream did not synchronise) */
	u32 *heads = (u32 *)h->scratch[0][s];
	const int rc = win_chain_launch(h, (const u8 *)d_in, n, chunk, nrec, d_plane, heads, (unsigned)cgrid,
					pheads ? (u32 *)((u8 *)heads + o_pheads) : NULL, seg_log, s);
	if (rc)
		return rc;
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_zstd_win_depth(int level) { return level < 10 ? 0 : level <= 12 ? 8 : level <= 15 ? 16 : level <= 18 ? 32 : 64; }

int gpumt_zstd_compress_batch_win(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				  size_t slot_stride, uint32_t *d_rec_len, int level, int s)
{
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > 0x40000000u || slot_stride < gpumt_zstd_slot_stride(chunk) ||
	    level < 1 || level > 22)
		return GPUMT_E_ARG;
	if (level < 10)
		return gpumt_zstd_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, level, s);
	if (use(h))
		return GPUMT_E_HIP;
	const size_t nrec = gpumt_lz4_record_count(n, chunk);
	const u32 bpr = (u32)((chunk + ZE_BLOCK - 1) / ZE_BLOCK);
	if (nrec * bpr > 0x7FFFFFFFu)
		return GPUMT_E_ARG;
	const u32 depth = h->zwin_depth ? (u32)h->zwin_depth : (u32)gpumt_zstd_win_depth(level);
	if (!h->zwin_waves) {
		int per_cu = 0;
		CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_zstd_enc_win_kernel, 64, 0));
		h->zwin_waves = (per_cu > 0 ? per_cu : 4) * (h->num_cus > 0 ? h->num_cus : 256);
	}
	/* slices of whole records, at most ZW_SLICE input bytes each; every slice sizes the same scratch */
	const size_t rps = chunk >= ZW_SLICE ? 1 : ZW_SLICE / chunk, slice_rec = nrec < rps ? nrec : rps;
	const size_t slice_in = slice_rec * chunk < n ? slice_rec * chunk : n, slice_blk = slice_rec * bpr;
	const size_t egrid = slice_blk < (size_t)h->zwin_waves ? slice_blk : (size_t)h->zwin_waves;
	const size_t cwaves = (size_t)4 * (h->num_cus > 0 ? h->num_cus : 256), cgrid = slice_rec < cwaves ? slice_rec : cwaves;
	const size_t o_seq = (slice_blk * 4 + 255) & ~(size_t)255, o_head = o_seq + ((egrid * ZE_WSCRATCH_BYTES + 255) & ~(size_t)255);
	const size_t o_plane = o_head + (cgrid * 4 << ZW_HLOG_MAX);
	const size_t need = (o_plane + GPUMT_ZSTD_WIN_SCRATCH(slice_in) + 0xFFFFF) & ~(size_t)0xFFFFF;
	/* chunks above 128 MiB carry a 128 KiB Window_Descriptor (zmt_zstd_assemble_kernel): the table encoder's */
	int win = chunk <= ZW_MAXDIST && !(h->zwin_refused && need >= h->zwin_refused);
	if (win && h->zwin_cap_mb && need > ((size_t)h->zwin_cap_mb << 20)) {
		h->zwin_refused = need;
		win = 0;
	}
	/* "win_chain_par": the plane + the head tables of the segment build are asked for first; refused, the serial kernel builds
	 * the plane and the rest of the call is as without the variant */
	const int seg_log = wchain_seg_log(h);
	const size_t pheads = win && seg_log ? gpumt_win_chain_par_scratch(slice_in, chunk, seg_log) : 0;
	int par = 0;
	if (pheads && (par = win_chain_par_ask(h, (need + pheads + 0xFFFFF) & ~(size_t)0xFFFFF, pheads, h->zwin_cap_mb, s)) < 0)
		return GPUMT_E_HIP;
	if (win && need > h->scratch_bytes[0][s]) {
		/* ask before letting go of the area the stream has: a refusal must leave the table encoder its scratch */
		void *p = dev_alloc(h, need);
		if (!p) {
			(void)hipGetLastError(); /* (a refused allocation is no error of this call) */
			h->zwin_refused = need;
			win = 0;
		} else {
			if (h->scratch[0][s]) {
				if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
					dev_free(h, p);
					return GPUMT_E_HIP;
				}
				dev_free(h, h->scratch[0][s]);
			}
			h->scratch[0][s] = p;
			h->scratch_bytes[0][s] = need;
		}
	}
	if (h->trace >= 1)
		fprintf(stderr, "[gpumt zstd win] records %zu depth %u plane %zu fallback %d\n", nrec, win ? depth : 0u,
			win ? (size_t)4 * slice_in : (size_t)0, win ? 0 : 1);
	if (h->trace >= 1 && win && seg_log)
		fprintf(stderr, "[gpumt win chain] segments %zu seg_log %d heads %zu serial %d\n",
			pheads ? slice_rec * (((slice_in < chunk ? slice_in : chunk) + ((size_t)1 << seg_log) - 1) >> seg_log) : slice_rec,
			seg_log, pheads, par ? 0 : 1);
	if (!win)
		return gpumt_zstd_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, level, s);
	u32 *blk_len = (u32 *)h->scratch[0][s];
	u8 *seqbuf = (u8 *)h->scratch[0][s] + o_seq;
	u32 *heads = (u32 *)((u8 *)h->scratch[0][s] + o_head), *plane = (u32 *)((u8 *)h->scratch[0][s] + o_plane);
	PROF0(9);
	for (size_t r0 = 0; r0 < nrec; r0 += slice_rec) {
		const size_t nr = nrec - r0 < slice_rec ? nrec - r0 : slice_rec, i0 = r0 * chunk;
		const size_t ni = n - i0 < nr * chunk ? n - i0 : nr * chunk, nb = nr * bpr;
		const unsigned eg = (unsigned)(nb < egrid ? nb : egrid), cg = (unsigned)(nr < cgrid ? nr : cgrid);
		const u8 *in = (const u8 *)d_in + i0;
		u8 *slots = (u8 *)d_slots + r0 * slot_stride;
		const int rc = win_chain_launch(h, in, ni, chunk, nr, plane, heads, cg, par ? (u32 *)((u8 *)h->scratch[0][s] + need) : NULL,
						seg_log, s);
		if (rc)
			return rc;
		hipLaunchKernelGGL(zmt_zstd_enc_win_kernel, dim3(eg), dim3(64), 0, h->st[s], in, (u64)ni, (u32)chunk, (u32)nb, bpr, slots,
				   (u64)slot_stride, blk_len, seqbuf, (const u32 *)plane, depth);
		hipLaunchKernelGGL(zmt_zstd_assemble_kernel, dim3((unsigned)nr), dim3(256), 0, h->st[s], (u64)ni, (u32)chunk, (u32)nr,
				   bpr, slots, (u64)slot_stride, (const u32 *)blk_len, d_rec_len + r0);
	}
	PROF1(9);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_zstd_probe_sizes(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
			   const uint32_t *d_rec_len, size_t nrec, uint32_t *d_out_len,
			   uint64_t *d_out_off, uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	hipLaunchKernelGGL(zmt_zstd_probe_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0,
			   h->st[s], (const u8 *)d_stream, d_rec_off, d_rec_len, (u32)nrec, d_out_len,
			   d_status);
	hipLaunchKernelGGL(zmt_scan_kernel, dim3(1), dim3(1024), 0, h->st[s],
			   (const u32 *)d_out_len, (u32)nrec, d_out_off);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* developer A/B: dynamic-LDS padding of the sequence pre-pass = a cap on its resident waves (GPUMT_ZSEQ_PAD, bytes) */
static size_t zseq_pad(void)
{
	static long v = -1;
	if (v < 0) {
		const char *e = getenv("GPUMT_ZSEQ_PAD");
		v = e && *e ? atol(e) : 0;
	}
	return (size_t)v;
}

/* The record decoders over the records whose `status` word is GPUMT_ST_OK.  gpumt_zstd_decompress_batch passes d_status and
 * no checksum words: they lie in the scratch and the verify pass follows.  gpumt_zstd_decompress_batch_par passes its
 * scratch copy of the status array and checksum words of its own (x_chk_e / x_chk_v), and runs the verify pass itself. */
static int zstd_decompress_records(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				   const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				   const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, u32 *x_chk_e, u32 *x_chk_v,
				   int s)
{
	/* per-record scratch (literals + sequences decoded ahead) is what bounds a launch: records go
	 * in slices of at most ZD_SLICE (5 GiB of scratch), each slice still 4x the resident waves */
	const size_t ZD_SLICE = 16384;
	const size_t slice = nrec < ZD_SLICE ? nrec : ZD_SLICE;
	const size_t lit_bytes = slice * (size_t)GPUMT_ZSTD_DEC_SCRATCH;
	/* the sequence pre-pass (zstd_dec_seq.hip) writes into a buffer as large as the output, record i at its d_out_off:
	 * only batches that can hold frames of more than one block have one */
	const size_t chk_bytes = (nrec * 8 + 64 + 15) & ~(size_t)15;
	const bool seq_on = h->zseq_variant == 0 && out_bytes / nrec > 131072;
	const size_t seq_bytes = seq_on ? out_bytes + 32 : 0;
	if (want_scratch(h, 1, s, lit_bytes + chk_bytes + seq_bytes))
		return GPUMT_E_HIP;
	u32 *chk_e = x_chk_e ? x_chk_e : (u32 *)((u8 *)h->scratch[1][s] + lit_bytes), *chk_v = x_chk_e ? x_chk_v : chk_e + nrec;
	/* the region's capacity goes to both kernels (zstd_dec_seq.h): records whose [out_off, out_off + out_len) does not fit
	 * out_bytes are decoded without the pre-pass instead of writing past the scratch */
	u8 *seqbuf = seq_on ? (u8 *)h->scratch[1][s] + lit_bytes + chk_bytes + 16 : NULL;
	const u64 seqcap = (u64)out_bytes;
	if (h->profile == 5 && !h->d_prof) {
		CK(hipMalloc((void **)&h->d_prof, 16 * sizeof(unsigned long long)));
		CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
	}
	PROF0(11);
	for (size_t b = 0; b < nrec; b += slice) {
		const size_t m = nrec - b < slice ? nrec - b : slice;
		if (seqbuf)
			hipLaunchKernelGGL(zmt_zstd_seq_kernel, dim3((unsigned)m), dim3(64), zseq_pad(), h->st[s],
					   (const u8 *)d_stream, (u64)stream_bytes, d_rec_off + b, d_rec_len + b, (u32)m,
					   d_out_off + b, (const u32 *)(d_out_len + b), (const u32 *)(d_status + b), seqbuf, seqcap);
		if (h->profile == 5) {
			hipLaunchKernelGGL(zmt_zstd_dec_kernel_prof, dim3((unsigned)m), dim3(64), 0, h->st[s],
					   (const u8 *)d_stream, (u64)stream_bytes, d_rec_off + b, d_rec_len + b, (u32)m,
					   (u8 *)d_out, d_out_off + b, d_out_len + b, (u8 *)h->scratch[1][s], d_status + b,
					   chk_e + b, chk_v + b, 0u, h->d_prof, seqbuf, seqcap);
		} else {
			/* small-table variant first (16 waves per CU); records that need the full-size tables
			 * come back with status 101 and are decoded by the general variant (12 waves per CU) */
			const u32 want = h->zdec_variant == 1 ? 0u : 101u;
			if (h->zdec_variant != 1)
				hipLaunchKernelGGL(zmt_zstd_dec_small_kernel, dim3((unsigned)m), dim3(64), 0, h->st[s],
						   (const u8 *)d_stream, (u64)stream_bytes, d_rec_off + b, d_rec_len + b, (u32)m,
						   (u8 *)d_out, d_out_off + b, d_out_len + b, (u8 *)h->scratch[1][s],
						   d_status + b, chk_e + b, chk_v + b, seqbuf, seqcap);
			hipLaunchKernelGGL(zmt_zstd_dec_kernel, dim3((unsigned)m), dim3(64), 0, h->st[s],
					   (const u8 *)d_stream, (u64)stream_bytes, d_rec_off + b, d_rec_len + b, (u32)m,
					   (u8 *)d_out, d_out_off + b, d_out_len + b, (u8 *)h->scratch[1][s], d_status + b,
					   chk_e + b, chk_v + b, want, seqbuf, seqcap);
		}
	}
	/* XXH64 content checksums, for the frames that carry one */
	if (!x_chk_e)
		hipLaunchKernelGGL(zmt_xxh64_verify_kernel, dim3((unsigned)((nrec * 4 + 255) / 256)), dim3(256), 0,
				   h->st[s], (const u8 *)d_out, d_out_off, (const u32 *)d_out_len, (u32)nrec, (const u32 *)chk_e,
				   (const u32 *)chk_v, d_status);
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_zstd_decompress_batch(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				const uint64_t *d_rec_off, const uint32_t *d_rec_len, size_t nrec,
				void *d_out, size_t out_bytes, const uint64_t *d_out_off,
				uint32_t *d_out_len, uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	return zstd_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
				       d_out_len, d_status, NULL, NULL, s);
}

int gpumt_zstd_decompress_blocks(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				 const gpumt_zstd_block *d_blocks, size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun,
				 void *d_out, size_t out_bytes, void *d_carry, uint32_t *d_run_len, uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || !d_stream || !d_blocks || !d_runs || !d_out || !d_carry || !d_run_len || !d_status ||
	    nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX || stream_bytes > 0xFFFFFFF0u)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* literal scratch per run bounds a launch: slices of at most ZR_SLICE runs (512 MiB of scratch) */
	const size_t ZR_SLICE = 4096;
	const size_t slice = nrun < ZR_SLICE ? nrun : ZR_SLICE;
	if (want_scratch(h, 1, s, slice * (size_t)GPUMT_ZSTD_RUN_SCRATCH))
		return GPUMT_E_HIP;
	PROF0(11);
	for (size_t b = 0; b < nrun; b += slice) {
		const size_t m = nrun - b < slice ? nrun - b : slice;
		hipLaunchKernelGGL(zmt_zstd_dec_run_kernel, dim3((unsigned)m), dim3(64), 0, h->st[s], (const u8 *)d_stream,
				   (u64)stream_bytes, d_blocks, (u32)nblk, d_runs + b, (u32)m, (u8 *)d_out, (u64)out_bytes,
				   (u8 *)d_carry, d_run_len + b, d_status + b, (u8 *)h->scratch[1][s]);
	}
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* scratch of the pre-pass, behind the runs' literal slots: slot | ZPre | def | mark per block (zstd_dec.hip) */
#define ZPRE_STRIDE ((size_t)GPUMT_ZSTD_PRE_SCRATCH(131072u))
#define ZPRE_REC 32u
int gpumt_zstd_decompress_blocks_pre(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				     const gpumt_zstd_block *d_blocks, size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun,
				     void *d_out, size_t out_bytes, void *d_carry, uint32_t *d_run_len, uint32_t *d_status,
				     uint32_t *d_block_mark, int s)
{
	if (!h || !STREAM_OK(s) || !d_stream || !d_blocks || !d_runs || !d_out || !d_carry || !d_run_len || !d_status ||
	    nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX || stream_bytes > 0xFFFFFFF0u)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* the execute stage reads the slots of all its blocks, so the runs go in one launch: a table whose runs or blocks
	 * would need more scratch than the device gives decodes serially */
	const size_t lit_bytes = (nrun * (size_t)GPUMT_ZSTD_RUN_SCRATCH + 255) & ~(size_t)255;
	const size_t pre_bytes = nblk * (ZPRE_STRIDE + ZPRE_REC + 16 + 4);
	const size_t need = (lit_bytes + pre_bytes + 0xFFFFF) & ~(size_t)0xFFFFF;
	int ahead = h->zrun_pre != 0 && nblk != 0 && nrun <= 4096 && !(h->zrun_pre_refused && need >= h->zrun_pre_refused);
	if (ahead && need > h->scratch_bytes[1][s]) {
		/* the larger area first, the current one dropped only once it is there: a refusal leaves the serial call its
		 * scratch, and a size the device has refused once is not asked for batch after batch */
		void *p = dev_alloc(h, need);
		if (!p) {
			(void)hipGetLastError(); /* (a refused allocation is no error of this call) */
			h->zrun_pre_refused = need;
			ahead = 0;
		} else {
			if (h->scratch[1][s]) {
				if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
					dev_free(h, p);
					return GPUMT_E_HIP;
				}
				dev_free(h, h->scratch[1][s]);
			}
			h->scratch[1][s] = p;
			h->scratch_bytes[1][s] = need;
		}
	}
	if (!ahead) {
		if (d_block_mark && nblk)
			CK(hipMemsetAsync(d_block_mark, 0, nblk * 4, h->st[s]));
		return gpumt_zstd_decompress_blocks(h, d_stream, stream_bytes, d_blocks, nblk, d_runs, nrun, d_out, out_bytes,
						    d_carry, d_run_len, d_status, s);
	}
	u8 *lit = (u8 *)h->scratch[1][s], *slots = lit + lit_bytes;
	void *pre = slots + nblk * ZPRE_STRIDE;
	u32 *def = (u32 *)((u8 *)pre + nblk * ZPRE_REC), *mark = def + 4 * nblk;
	PROF0(11);
	hipLaunchKernelGGL(zmt_zstd_pre_classify_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, h->st[s],
			   (const u8 *)d_stream, (u64)stream_bytes, d_blocks, (u32)nblk, pre, def, mark);
	hipLaunchKernelGGL(zmt_zstd_pre_resolve_kernel, dim3((unsigned)nrun), dim3(64), 0, h->st[s], d_runs, (u32)nrun, (u32)nblk,
			   (const void *)pre, def, (u32 *)nullptr);
	hipLaunchKernelGGL(zmt_zstd_pre_entropy_kernel, dim3((unsigned)nblk), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, (const void *)pre, (const u32 *)def, slots, mark);
	hipLaunchKernelGGL(zmt_zstd_dec_run_pre_kernel, dim3((unsigned)nrun), dim3(64), 0, h->st[s], (const u8 *)d_stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, d_runs, (u32)nrun, (u8 *)d_out, (u64)out_bytes, (u8 *)d_carry,
			   d_run_len, d_status, lit, (const u32 *)mark, (const u32 *)def, (const u8 *)slots);
	if (d_block_mark)
		CK(hipMemcpyAsync(d_block_mark, mark, nblk * 4, hipMemcpyDeviceToDevice, h->st[s]));
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_zstd_decompress_blocks_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				     const gpumt_zstd_block *d_blocks, size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun,
				     void *d_out, size_t out_bytes, void *d_carry, uint32_t *d_run_len, uint32_t *d_status,
				     uint32_t *d_block_mark, uint32_t *d_block_par, int s)
{
	if (!h || !STREAM_OK(s) || !d_stream || !d_blocks || !d_runs || !d_out || !d_carry || !d_run_len || !d_status ||
	    nrun == 0 || nrun > GPUMT_LZ4_BLOCKS_MAX || nblk > GPUMT_LZ4_BLOCKS_MAX || stream_bytes > 0xFFFFFFF0u)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	/* the pre-pass scratch, then the origin plane (one u32 per byte of d_out), a run record, a carry copy and 13 words per
	 * run, 12 words per block */
	const size_t lit_bytes = (nrun * (size_t)GPUMT_ZSTD_RUN_SCRATCH + 255) & ~(size_t)255;
	const size_t pre_bytes = (nblk * (ZPRE_STRIDE + ZPRE_REC + 16 + 4) + 255) & ~(size_t)255;
	const size_t plane = (GPUMT_ZSTD_PAR_SCRATCH(out_bytes) + 255) & ~(size_t)255;
	const size_t run_bytes = (nrun * (sizeof(gpumt_zstd_run) + (size_t)GPUMT_ZSTD_CARRY_BYTES + 13 * 4) + 255) & ~(size_t)255;
	const size_t need = (lit_bytes + pre_bytes + plane + run_bytes + nblk * 12 * 4 + 256 + 0xFFFFF) & ~(size_t)0xFFFFF;
	/* a table without a run of two blocks has nothing to decode side by side */
	int par = h->zrun_par != 0 && h->zrun_pre != 0 && nblk > nrun && nrun <= 4096 &&
		  !(h->zrun_par_refused && need >= h->zrun_par_refused);
	if (par && need > h->scratch_bytes[1][s]) {
		/* as gpumt_zstd_decompress_blocks_pre: the larger area first, a refused size is not asked for again */
		void *p = dev_alloc(h, need);
		if (!p) {
			(void)hipGetLastError(); /* (a refused allocation is no error of this call) */
			h->zrun_par_refused = need;
			par = 0;
		} else {
			if (h->scratch[1][s]) {
				if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
					dev_free(h, p);
					return GPUMT_E_HIP;
				}
				dev_free(h, h->scratch[1][s]);
			}
			h->scratch[1][s] = p;
			h->scratch_bytes[1][s] = need;
		}
	}
	if (!par) {
		if (d_block_par && nblk)
			CK(hipMemsetAsync(d_block_par, 0, nblk * 4, h->st[s]));
		return gpumt_zstd_decompress_blocks_pre(h, d_stream, stream_bytes, d_blocks, nblk, d_runs, nrun, d_out, out_bytes,
							d_carry, d_run_len, d_status, d_block_mark, s);
	}
	u8 *lit = (u8 *)h->scratch[1][s], *slots = lit + lit_bytes;
	void *pre = slots + nblk * ZPRE_STRIDE;
	u32 *def = (u32 *)((u8 *)pre + nblk * ZPRE_REC), *mark = def + 4 * nblk;
	ZPar P;
	P.origin = (u32 *)(lit + lit_bytes + pre_bytes);
	P.prun = (gpumt_zstd_run *)((u8 *)P.origin + plane);
	P.pcarry = (u8 *)(P.prun + nrun);
	P.sfx = (u32 *)(P.pcarry + nrun * (size_t)GPUMT_ZSTD_CARRY_BYTES);
	P.rflag = P.sfx + nrun;
	P.plen = P.rflag + nrun;
	P.pst = P.plen + nrun;
	P.rrep = P.pst + nrun;
	P.rlen = P.rrep + 3 * nrun;
	P.rlast = P.rlen + nrun;
	P.owner = (u32 *)((u8 *)P.prun + run_bytes);
	P.blen = P.owner + nblk;
	P.bst = P.blen + nblk;
	P.btf = P.bst + nblk;
	P.bpos = P.btf + 3 * nblk;
	P.brep = P.bpos + nblk;
	P.xst = P.brep + 3 * nblk;
	u32 *par_out = P.xst + nblk; /* block_par, where the caller wants none */
	P.flag = par_out + nblk;
	if (d_block_par)
		par_out = d_block_par;
	const hipStream_t st = h->st[s];
	const dim3 wave(64), per_run((unsigned)nrun), per_blk((unsigned)nblk);
	const u8 *stream = (const u8 *)d_stream;
	PROF0(11);
	CK(hipMemsetAsync(P.owner, 0xFF, nblk * 4, st));
	CK(hipMemsetAsync(P.flag, 0, 4, st));
	CK(hipMemsetAsync(par_out, 0, nblk * 4, st));
	hipLaunchKernelGGL(zmt_zstd_pre_classify_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, stream,
			   (u64)stream_bytes, d_blocks, (u32)nblk, pre, def, mark);
	hipLaunchKernelGGL(zmt_zstd_pre_resolve_kernel, per_run, wave, 0, st, d_runs, (u32)nrun, (u32)nblk, (const void *)pre, def,
			   P.rlast);
	hipLaunchKernelGGL(zmt_zstd_pre_entropy_kernel, per_blk, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk,
			   (const void *)pre, (const u32 *)def, slots, mark);
	hipLaunchKernelGGL(zmt_zstd_par_plan_kernel, dim3(1), wave, 0, st, d_runs, (u32)nrun, (u32)nblk, (u64)out_bytes, P);
	hipLaunchKernelGGL(zmt_zstd_par_split_kernel, per_run, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk, d_runs,
			   (u32)nrun, (u64)out_bytes, (const u32 *)mark, P);
	hipLaunchKernelGGL(zmt_zstd_par_prefix_kernel, per_run, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk, d_runs,
			   (u32)nrun, (u8 *)d_out, (u64)out_bytes, (const u8 *)d_carry, lit, (const u32 *)mark, (const u32 *)def,
			   (const u8 *)slots, P);
	hipLaunchKernelGGL(zmt_zstd_par_measure_kernel, per_blk, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk, d_runs,
			   (const void *)pre, (const u32 *)mark, (const u8 *)slots, P);
	hipLaunchKernelGGL(zmt_zstd_par_scan_kernel, per_run, wave, 0, st, d_runs, (u32)nrun, P);
	hipLaunchKernelGGL(zmt_zstd_par_exec_kernel, per_blk, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk, d_runs,
			   (const void *)pre, slots, (u8 *)d_out, P);
	hipLaunchKernelGGL(zmt_zstd_par_resolve_kernel, per_run, dim3(1024), 0, st, d_runs, (u32)nrun, (u8 *)d_out, P);
	hipLaunchKernelGGL(zmt_zstd_par_fallback_kernel, per_run, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk,
			   d_runs, (u32)nrun, (u8 *)d_out, (u64)out_bytes, (u8 *)d_carry, d_run_len, d_status, lit,
			   (const u32 *)mark, (const u32 *)def, (const u8 *)slots, P);
	hipLaunchKernelGGL(zmt_zstd_par_carry_kernel, per_run, wave, 0, st, stream, (u64)stream_bytes, d_blocks, (u32)nblk, d_runs,
			   (u32)nrun, (const void *)pre, (u8 *)d_carry, d_run_len, d_status, par_out, P);
	if (d_block_mark)
		CK(hipMemcpyAsync(d_block_mark, mark, nblk * 4, hipMemcpyDeviceToDevice, st));
	PROF1(11);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* grow one of the record stage's areas (never shrinks): the larger area first, the current one dropped only once it is
 * there.  -> nonzero when the device refuses */
static int zrec_want(gpumt_ctx *h, void **area, size_t *have, size_t bytes, hipStream_t st)
{
	if (bytes <= *have)
		return 0;
	bytes = (bytes + 0xFFFFF) & ~(size_t)0xFFFFF;
	void *p = dev_alloc(h, bytes);
	if (!p) {
		(void)hipGetLastError(); /* (a refused allocation is no error of the call) */
		return 1;
	}
	if (*area) {
		if (hipStreamSynchronize(st) != hipSuccess) {
			dev_free(h, p);
			return 1;
		}
		dev_free(h, *area);
	}
	*area = p;
	*have = bytes;
	return 0;
}

int gpumt_zstd_decompress_batch_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				    const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				    const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int s)
{
	static_assert(sizeof(ZRec) == 56, "record layout");
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	const hipStream_t st = h->st[s];
	if (d_rec_par)
		CK(hipMemsetAsync(d_rec_par, 0, nrec * 4, st));
	if (!h->zrec_par) {
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt zstd rec] records %zu par 0 blocks 0 slices 0 fallback 0\n", nrec);
		return zstd_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					       d_out_len, d_status, NULL, NULL, s);
	}
	/* the stage's own areas, which the block call and the record decoders do not replace.  Per record: the counts and five
	 * words (scratch status, checksum expected / valid, first block, run).  Per slice, sized once the counts are known: the
	 * block table, the run table with length and status per run, and a carry area no run touches */
	const size_t rec_bytes = (nrec * sizeof(ZRec) + 255) & ~(size_t)255, word_bytes = (nrec * 4 + 255) & ~(size_t)255;
	const size_t need_a = rec_bytes + 5 * word_bytes;
	const size_t cap = h->zrec_cap_mb ? (size_t)h->zrec_cap_mb << 20 : ~(size_t)0;
	int par = !(h->zrec_refused && need_a >= h->zrec_refused);
	if (par && need_a > cap) {
		h->zrec_refused = need_a;
		par = 0;
	}
	if (par && zrec_want(h, &h->zrec_area[s], &h->zrec_bytes[s], need_a, st)) {
		h->zrec_refused = need_a;
		par = 0;
	}
	if (par && rec_bytes > h->zrec_pin_bytes[s]) {
		/* (the copy that read the old area was waited for by the call that queued it) */
		void *p = NULL;
		if (hipHostMalloc(&p, rec_bytes, hipHostMallocDefault) != hipSuccess || !p) {
			(void)hipGetLastError();
			h->zrec_refused = need_a;
			par = 0;
		} else {
			if (h->zrec_pin[s])
				(void)hipHostFree(h->zrec_pin[s]);
			h->zrec_pin[s] = p;
			h->zrec_pin_bytes[s] = rec_bytes;
		}
	}
	if (!par) {
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt zstd rec] records %zu par 0 blocks 0 slices 0 fallback 1\n", nrec);
		return zstd_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					       d_out_len, d_status, NULL, NULL, s);
	}
	u8 *area = (u8 *)h->zrec_area[s];
	ZRec *recs = (ZRec *)area;
	u32 *sstatus = (u32 *)(area + rec_bytes), *chk_e = (u32 *)((u8 *)sstatus + word_bytes);
	u32 *chk_v = (u32 *)((u8 *)chk_e + word_bytes), *rfirst = (u32 *)((u8 *)chk_v + word_bytes);
	u32 *rrun = (u32 *)((u8 *)rfirst + word_bytes);
	const u8 *stream = (const u8 *)d_stream;
	const dim3 per_rec((unsigned)((nrec + 255) / 256)), tpb(256);
	hipLaunchKernelGGL(zmt_zstd_rec_count_kernel, per_rec, tpb, 0, st, stream, (u64)stream_bytes, d_rec_off, d_rec_len, (u32)nrec,
			   d_out_off, (const u32 *)d_out_len, (u64)out_bytes, (const u32 *)d_status, (u32)h->zrec_min_blocks, recs);
	/* one round trip: the host sizes the tables and the launches of the block stages from the counts */
	const ZRec *hrec = (const ZRec *)h->zrec_pin[s];
	CK(hipMemcpyAsync(h->zrec_pin[s], recs, nrec * sizeof(ZRec), hipMemcpyDeviceToHost, st));
	CK(hipStreamSynchronize(st));
	const u32 SB = (u32)h->zrec_slice_blocks;
	size_t npar = 0, nblocks = 0, nslices = 0, max_blk = 0, max_run = 0;
	ZRecSlice S;
	for (size_t at = 0; zrec_next_slice(hrec, nrec, at, SB, &S); at = S.b) {
		npar += S.nrun;
		nblocks += S.nblk;
		nslices++;
		max_blk = S.nblk > max_blk ? S.nblk : max_blk;
		max_run = S.nrun > max_run ? S.nrun : max_run;
	}
	const size_t blk_bytes = (max_blk * sizeof(gpumt_zstd_block) + 255) & ~(size_t)255;
	const size_t run_bytes = (max_run * (sizeof(gpumt_zstd_run) + 8) + 255) & ~(size_t)255;
	const size_t need_b = blk_bytes + run_bytes + 2 * (size_t)GPUMT_ZSTD_CARRY_BYTES, need = need_a + need_b;
	if (nslices && ((h->zrec_refused && need >= h->zrec_refused) || need > cap ||
			zrec_want(h, &h->zrec_tab[s], &h->zrec_tab_bytes[s], need_b, st))) {
		h->zrec_refused = need;
		par = 0;
	}
	if (!par || !nslices) {
		/* nothing for the block stages (or no room for their tables): the record decoders, on d_status itself */
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt zstd rec] records %zu par 0 blocks 0 slices 0 fallback %d\n", nrec, par ? 0 : 1);
		return zstd_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					       d_out_len, d_status, NULL, NULL, s);
	}
	gpumt_zstd_block *blocks = (gpumt_zstd_block *)h->zrec_tab[s];
	gpumt_zstd_run *runs = (gpumt_zstd_run *)((u8 *)blocks + blk_bytes);
	u32 *run_len = (u32 *)(runs + max_run), *run_st = run_len + max_run;
	u8 *carry = (u8 *)blocks + blk_bytes + run_bytes;
	CK(hipMemcpyAsync(sstatus, d_status, nrec * 4, hipMemcpyDeviceToDevice, st));
	CK(hipMemsetAsync(chk_v, 0, nrec * 4, st));
	for (size_t at = 0; zrec_next_slice(hrec, nrec, at, SB, &S); at = S.b) {
		const u32 n = (u32)(S.b - S.a);
		hipLaunchKernelGGL(zmt_zstd_rec_scan_kernel, dim3(1), tpb, 0, st, (const ZRec *)(recs + S.a), n, rfirst + S.a,
				   rrun + S.a);
		hipLaunchKernelGGL(zmt_zstd_rec_table_kernel, dim3((n + 255) / 256), tpb, 0, st, stream, (const ZRec *)(recs + S.a), n,
				   (const u32 *)(rfirst + S.a), (const u32 *)(rrun + S.a), S.in_lo, S.out_lo, S.nblk, S.nrun, blocks,
				   runs);
		/* the existing call, with d_stream and d_out at the slice: its origin plane is 4 x the slice's output span */
		const int rc = gpumt_zstd_decompress_blocks_par(h, stream + S.in_lo, (size_t)(S.in_hi - S.in_lo), blocks, S.nblk, runs,
								S.nrun, (u8 *)d_out + S.out_lo, (size_t)(S.out_hi - S.out_lo), carry,
								run_len, run_st, NULL, NULL, s);
		if (rc != GPUMT_OK)
			return rc;
		hipLaunchKernelGGL(zmt_zstd_rec_finish_kernel, dim3((n + 255) / 256), tpb, 0, st, stream, (const ZRec *)(recs + S.a), n,
				   (const u32 *)(rrun + S.a), S.nrun, (const u32 *)run_len, (const u32 *)run_st, d_out_len + S.a,
				   d_rec_par ? d_rec_par + S.a : (u32 *)NULL, sstatus + S.a, chk_e + S.a, chk_v + S.a);
	}
	if (h->trace >= 1)
		fprintf(stderr, "[gpumt zstd rec] records %zu par %zu blocks %zu slices %zu fallback 0\n", nrec, npar, nblocks,
			nslices);
	/* everything the block stages did not keep is decoded and judged by the record decoders */
	const int rc = zstd_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					       d_out_len, sstatus, chk_e, chk_v, s);
	if (rc != GPUMT_OK)
		return rc;
	hipLaunchKernelGGL(zmt_zstd_rec_merge_kernel, per_rec, tpb, 0, st, (const u32 *)sstatus, (u32)nrec, d_status);
	hipLaunchKernelGGL(zmt_xxh64_verify_kernel, dim3((unsigned)((nrec * 4 + 255) / 256)), tpb, 0, st, (const u8 *)d_out,
			   d_out_off, (const u32 *)d_out_len, (u32)nrec, (const u32 *)chk_e, (const u32 *)chk_v, d_status);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* gpumt_zstd_decompress_batch_par's structure with the LZ4 block calls behind it (lz4_dec_rec.h) */
int gpumt_lz4_decompress_batch_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes, const uint64_t *d_rec_off,
				   const uint32_t *d_rec_len, size_t nrec, void *d_out, size_t out_bytes,
				   const uint64_t *d_out_off, uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int s)
{
	static_assert(sizeof(LRec) == 56, "record layout");
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	const hipStream_t st = h->st[s];
	const int seg = h->lrec_seg;
	const char *route = seg ? "seg" : "par";
	if (d_rec_par)
		CK(hipMemsetAsync(d_rec_par, 0, nrec * 4, st));
	if (!h->lrec_par) {
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt lz4 rec] records %zu par 0 blocks 0 slices 0 fallback 0 route %s\n", nrec, route);
		return lz4_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					      d_out_len, d_status, NULL, NULL, NULL, s);
	}
	/* the stage's own areas, which the block calls and the record decoders do not replace.  Per record: the counts and five
	 * words (scratch status = the record decoders' kept array, checksum expected / valid, first block, run).  Per slice,
	 * sized once the counts are known: the block table with length and segment count per block, and the run table with
	 * length and status per run */
	const size_t rec_bytes = (nrec * sizeof(LRec) + 255) & ~(size_t)255, word_bytes = (nrec * 4 + 255) & ~(size_t)255;
	const size_t need_a = rec_bytes + 5 * word_bytes;
	const size_t cap = h->lrec_cap_mb ? (size_t)h->lrec_cap_mb << 20 : ~(size_t)0;
	int par = !(h->lrec_refused && need_a >= h->lrec_refused);
	if (par && need_a > cap) {
		h->lrec_refused = need_a;
		par = 0;
	}
	if (par && zrec_want(h, &h->lrec_area[s], &h->lrec_bytes[s], need_a, st)) {
		h->lrec_refused = need_a;
		par = 0;
	}
	if (par && rec_bytes > h->lrec_pin_bytes[s]) {
		/* (the copy that read the old area was waited for by the call that queued it) */
		void *p = NULL;
		if (hipHostMalloc(&p, rec_bytes, hipHostMallocDefault) != hipSuccess || !p) {
			(void)hipGetLastError();
			h->lrec_refused = need_a;
			par = 0;
		} else {
			if (h->lrec_pin[s])
				(void)hipHostFree(h->lrec_pin[s]);
			h->lrec_pin[s] = p;
			h->lrec_pin_bytes[s] = rec_bytes;
		}
	}
	if (!par) {
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt lz4 rec] records %zu par 0 blocks 0 slices 0 fallback 1 route %s\n", nrec, route);
		return lz4_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					      d_out_len, d_status, NULL, NULL, NULL, s);
	}
	u8 *area = (u8 *)h->lrec_area[s];
	LRec *recs = (LRec *)area;
	u32 *sstatus = (u32 *)(area + rec_bytes), *chk_e = (u32 *)((u8 *)sstatus + word_bytes);
	u32 *chk_v = (u32 *)((u8 *)chk_e + word_bytes), *rfirst = (u32 *)((u8 *)chk_v + word_bytes);
	u32 *rrun = (u32 *)((u8 *)rfirst + word_bytes);
	const u8 *stream = (const u8 *)d_stream;
	const dim3 per_rec((unsigned)((nrec + 255) / 256)), tpb(256);
	hipLaunchKernelGGL(zmt_lz4_rec_count_kernel, per_rec, tpb, 0, st, stream, (u64)stream_bytes, d_rec_off, d_rec_len, (u32)nrec,
			   d_out_off, (const u32 *)d_out_len, (u64)out_bytes, (u32)h->lrec_min_blocks, seg ? (u32)h->lseg_bytes : 0u,
			   recs);
	/* one round trip: the host sizes the tables and the launches of the block stages from the counts */
	const LRec *hrec = (const LRec *)h->lrec_pin[s];
	CK(hipMemcpyAsync(h->lrec_pin[s], recs, nrec * sizeof(LRec), hipMemcpyDeviceToHost, st));
	CK(hipStreamSynchronize(st));
	const u32 SB = (u32)h->lrec_slice_blocks;
	size_t npar = 0, nblocks = 0, nslices = 0, max_blk = 0, max_run = 0;
	LRecSlice S;
	for (size_t at = 0; lrec_next_slice(hrec, nrec, at, SB, &S); at = S.b) {
		npar += S.nrun;
		nblocks += S.nblk;
		nslices++;
		max_blk = S.nblk > max_blk ? S.nblk : max_blk;
		max_run = S.nrun > max_run ? S.nrun : max_run;
	}
	const size_t blk_bytes = (max_blk * (sizeof(gpumt_lz4_block) + 8) + 255) & ~(size_t)255;
	const size_t run_bytes = (max_run * (sizeof(gpumt_lz4_run) + 8) + 255) & ~(size_t)255;
	const size_t need_b = blk_bytes + run_bytes, need = need_a + need_b;
	if (nslices && ((h->lrec_refused && need >= h->lrec_refused) || need > cap ||
			zrec_want(h, &h->lrec_tab[s], &h->lrec_tab_bytes[s], need_b, st))) {
		h->lrec_refused = need;
		par = 0;
	}
	if (!par || !nslices) {
		/* nothing for the block stages (or no room for their tables): the record decoders alone */
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt lz4 rec] records %zu par 0 blocks 0 slices 0 fallback %d route %s\n", nrec, par ? 0 : 1,
				route);
		return lz4_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					      d_out_len, d_status, NULL, NULL, NULL, s);
	}
	gpumt_lz4_block *blocks = (gpumt_lz4_block *)h->lrec_tab[s];
	u32 *blk_len = (u32 *)(blocks + max_blk), *blk_seg = blk_len + max_blk;
	gpumt_lz4_run *runs = (gpumt_lz4_run *)((u8 *)blocks + blk_bytes);
	u32 *run_len = (u32 *)(runs + max_run), *run_st = run_len + max_run;
	CK(hipMemsetAsync(sstatus, 0, nrec * 4, st));
	CK(hipMemsetAsync(chk_v, 0, nrec * 4, st));
	/* the slices first, the record pass after them: the block calls replace scratch[1][s], which the record pass carves up */
	for (size_t at = 0; lrec_next_slice(hrec, nrec, at, SB, &S); at = S.b) {
		const u32 n = (u32)(S.b - S.a);
		hipLaunchKernelGGL(zmt_lz4_rec_scan_kernel, dim3(1), tpb, 0, st, (const LRec *)(recs + S.a), n, rfirst + S.a, rrun + S.a);
		hipLaunchKernelGGL(zmt_lz4_rec_table_kernel, dim3((n + 255) / 256), tpb, 0, st, stream, (const LRec *)(recs + S.a), n,
				   (const u32 *)(rfirst + S.a), (const u32 *)(rrun + S.a), S.in_lo, S.out_lo, S.nblk, S.nrun, blocks,
				   runs);
		/* the existing call, with d_stream and d_out at the slice: its origin plane is 2 x the slice's output span */
		const int rc = seg ? gpumt_lz4_decompress_blocks_seg(h, stream + S.in_lo, (size_t)(S.in_hi - S.in_lo), blocks, S.nblk,
								     runs, S.nrun, (u8 *)d_out + S.out_lo,
								     (size_t)(S.out_hi - S.out_lo), blk_len, run_len, run_st, blk_seg, s)
				   : gpumt_lz4_decompress_blocks_par(h, stream + S.in_lo, (size_t)(S.in_hi - S.in_lo), blocks, S.nblk,
								     runs, S.nrun, (u8 *)d_out + S.out_lo,
								     (size_t)(S.out_hi - S.out_lo), blk_len, run_len, run_st, s);
		if (rc != GPUMT_OK)
			return rc;
		hipLaunchKernelGGL(zmt_lz4_rec_finish_kernel, dim3((n + 255) / 256), tpb, 0, st, stream, (const LRec *)(recs + S.a), n,
				   (const u32 *)(rrun + S.a), S.nrun, (const u32 *)run_len, (const u32 *)run_st, d_out_len + S.a,
				   d_rec_par ? d_rec_par + S.a : (u32 *)NULL, sstatus + S.a, chk_e + S.a, chk_v + S.a);
	}
	if (h->trace >= 1)
		fprintf(stderr, "[gpumt lz4 rec] records %zu par %zu blocks %zu slices %zu fallback 0 route %s\n", nrec, npar, nblocks,
			nslices, route);
	/* everything the block stages did not keep is decoded and judged by the record decoders */
	const int rc = lz4_decompress_records(h, d_stream, stream_bytes, d_rec_off, d_rec_len, nrec, d_out, out_bytes, d_out_off,
					      d_out_len, d_status, (const u32 *)sstatus, chk_e, chk_v, s);
	if (rc != GPUMT_OK)
		return rc;
	hipLaunchKernelGGL(zmt_lz4_rec_merge_kernel, per_rec, tpb, 0, st, (const u32 *)sstatus, (u32)nrec, d_status, d_rec_par);
	hipLaunchKernelGGL(zmt_xxh32_kernel, dim3((unsigned)((nrec * 4 + 255) / 256)), tpb, 0, st, (const u8 *)d_out, d_out_off,
			   (const u32 *)d_out_len, (u32)nrec, (u32 *)NULL, (const u32 *)chk_e, (const u32 *)chk_v, d_status);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_xxh64_carry(gpumt_ctx *h, const void *d_base, size_t base_bytes, const gpumt_xxh32_job *d_jobs, size_t njobs,
		      uint32_t *d_states, uint32_t *d_digest, uint32_t *d_verdict, int s)
{
	if (!h || !STREAM_OK(s) || !d_base || !d_jobs || !d_states || !d_digest || !d_verdict || njobs > GPUMT_LZ4_BLOCKS_MAX)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!njobs)
		return GPUMT_OK;
	PROF0(12);
	hipLaunchKernelGGL(zmt_xxh64_carry_kernel, dim3((unsigned)njobs), dim3(64), 0, h->st[s], (const u8 *)d_base,
			   (u64)base_bytes, d_jobs, (u32)njobs, d_states, d_digest, d_verdict);
	PROF1(12);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* brotli-mt compress: same slot geometry as zstd (gpumt_zstd_slot_stride), 16-byte record headers */
/* quality -> encoder tier (brotli_enc.hip): 0-3 the fast parse (4 Ki-entry table), 4-8 and 9-11 larger tables and
 * minimum match 6 */
int gpumt_brotli_level_tier(int level) { return level <= 3 ? 0 : level <= 8 ? 1 : 2; }

int gpumt_brotli_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				size_t slot_stride, uint32_t *d_rec_len, int s)
{
	return gpumt_brotli_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, 1, s);
}

static int brotli_compress_tables(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots, size_t slot_stride,
				  uint32_t *d_rec_len, int level, int index, int s);

int gpumt_brotli_compress_batch_level(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				      size_t slot_stride, uint32_t *d_rec_len, int level, int s)
{
	return brotli_compress_tables(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, level, 0, s);
}

/* the same records with the span index of brotli_dec_rec.h in those of two blocks or more */
int gpumt_brotli_compress_batch_index(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				      size_t slot_stride, uint32_t *d_rec_len, int level, int s)
{
	return brotli_compress_tables(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, level, 1, s);
}

static int brotli_compress_tables(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots, size_t slot_stride,
				  uint32_t *d_rec_len, int level, int index, int s)
{
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > 0x40000000u || slot_stride < gpumt_zstd_slot_stride(chunk) ||
	    level < 0 || level > 11)
		return GPUMT_E_ARG;
	const int tier = gpumt_brotli_level_tier(level);
	if (use(h))
		return GPUMT_E_HIP;
	const size_t nrec = gpumt_lz4_record_count(n, chunk);
	const u32 bpr = (u32)((chunk + ZE_BLOCK - 1) / ZE_BLOCK);
	const size_t nblk = nrec * bpr;
	if (nblk > 0x7FFFFFFFu)
		return GPUMT_E_ARG;
	if (!h->benc_waves[tier]) {
		int per_cu = 0;
		if (tier == 0)
			CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_brotli_enc_kernel, 64, 0));
		else if (tier == 1)
			CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_brotli_enc_t2_kernel, 64, 0));
		else
			CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_brotli_enc_t3_kernel, 64, 0));
		h->benc_waves[tier] = (per_cu > 0 ? per_cu : 4) * (h->num_cus > 0 ? h->num_cus : 256);
		if (getenv("GPUMT_VERBOSE"))
			fprintf(stderr, "gpumt: brotli encoder tier %d grid %d waves\n", tier, h->benc_waves[tier]);
	}
	const unsigned grid = (unsigned)(nblk < (size_t)h->benc_waves[tier] ? nblk : (size_t)h->benc_waves[tier]);
	const size_t seq_bytes = (size_t)grid * (3 * ZE_MAXSEQ * 4);
	if (want_scratch(h, 0, s, nblk * 4 + 64 + seq_bytes))
		return GPUMT_E_HIP;
	u32 *blk_len = (u32 *)h->scratch[0][s];
	u8 *seqbuf = (u8 *)h->scratch[0][s] + ((nblk * 4 + 63) & ~(size_t)63);
	PROF0(9);
	if (tier == 0)
		hipLaunchKernelGGL(zmt_brotli_enc_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
				   (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len, seqbuf);
	else if (tier == 1)
		hipLaunchKernelGGL(zmt_brotli_enc_t2_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
				   (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len, seqbuf);
	else
		hipLaunchKernelGGL(zmt_brotli_enc_t3_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
				   (u32)chunk, (u32)nblk, bpr, (u8 *)d_slots, (u64)slot_stride, blk_len, seqbuf);
	if (index)
		hipLaunchKernelGGL(zmt_brotli_assemble_index_kernel, dim3((unsigned)nrec), dim3(256), 0, h->st[s], (u64)n,
				   (u32)chunk, (u32)nrec, bpr, (u8 *)d_slots, (u64)slot_stride, (const u32 *)blk_len,
				   d_rec_len);
	else
		hipLaunchKernelGGL(zmt_brotli_assemble_kernel, dim3((unsigned)nrec), dim3(256), 0, h->st[s], (u64)n,
				   (u32)chunk, (u32)nrec, bpr, (u8 *)d_slots, (u64)slot_stride, (const u32 *)blk_len,
				   d_rec_len);
	PROF1(9);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* ---- the whole chunk as the match window (brotli_enc_win.h): the chain plane is the zstd encoder's ---- */
int gpumt_brotli_win_depth(int level) { return level < 9 ? 0 : level == 9 ? 16 : level == 10 ? 32 : 64; }

int gpumt_brotli_compress_batch_win(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				    size_t slot_stride, uint32_t *d_rec_len, int level, int s)
{
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > 0x40000000u || slot_stride < gpumt_zstd_slot_stride(chunk) ||
	    level < 0 || level > 11)
		return GPUMT_E_ARG;
	if (level < 9)
		return gpumt_brotli_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, level, s);
	if (use(h))
		return GPUMT_E_HIP;
	const size_t nrec = gpumt_lz4_record_count(n, chunk);
	const u32 bpr = (u32)((chunk + ZE_BLOCK - 1) / ZE_BLOCK);
	if (nrec * bpr > 0x7FFFFFFFu)
		return GPUMT_E_ARG;
	const u32 depth = h->bwin_depth ? (u32)h->bwin_depth : (u32)gpumt_brotli_win_depth(level);
	if (!h->bwin_waves) {
		int per_cu = 0;
		CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_brotli_enc_win_kernel, 64, 0));
		h->bwin_waves = (per_cu > 0 ? per_cu : 4) * (h->num_cus > 0 ? h->num_cus : 256);
	}
	/* slices of whole records, at most ZW_SLICE input bytes each; every slice sizes the same scratch */
	const size_t rps = chunk >= ZW_SLICE ? 1 : ZW_SLICE / chunk, slice_rec = nrec < rps ? nrec : rps;
	const size_t slice_in = slice_rec * chunk < n ? slice_rec * chunk : n, slice_blk = slice_rec * bpr;
	const size_t egrid = slice_blk < (size_t)h->bwin_waves ? slice_blk : (size_t)h->bwin_waves;
	const size_t cwaves = (size_t)4 * (h->num_cus > 0 ? h->num_cus : 256), cgrid = slice_rec < cwaves ? slice_rec : cwaves;
	const size_t o_seq = (slice_blk * 4 + 255) & ~(size_t)255;
	const size_t o_head = o_seq + ((egrid * ((size_t)3 * ZE_MAXSEQ * 4) + 255) & ~(size_t)255);
	const size_t o_plane = o_head + (cgrid * 4 << ZW_HLOG_MAX);
	const size_t need = (o_plane + GPUMT_BROTLI_WIN_SCRATCH(slice_in) + 0xFFFFF) & ~(size_t)0xFFFFF;
	int win = !(h->bwin_refused && need >= h->bwin_refused);
	if (win && h->bwin_cap_mb && need > ((size_t)h->bwin_cap_mb << 20)) {
		h->bwin_refused = need;
		win = 0;
	}
	/* "win_chain_par": the plane + the head tables of the segment build are asked for first; refused, the serial kernel builds
	 * the plane and the rest of the call is as without the variant */
	const int seg_log = wchain_seg_log(h);
	const size_t pheads = win && seg_log ? gpumt_win_chain_par_scratch(slice_in, chunk, seg_log) : 0;
	int par = 0;
	if (pheads && (par = win_chain_par_ask(h, (need + pheads + 0xFFFFF) & ~(size_t)0xFFFFF, pheads, h->bwin_cap_mb, s)) < 0)
		return GPUMT_E_HIP;
	if (win && need > h->scratch_bytes[0][s]) {
		/* ask before letting go of the area the stream has: a refusal must leave the table encoder its scratch */
		void *p = dev_alloc(h, need);
		if (!p) {
			(void)hipGetLastError(); /* (a refused allocation is no error of this call) */
			h->bwin_refused = need;
			win = 0;
		} else {
			if (h->scratch[0][s]) {
				if (hipStreamSynchronize(h->st[s]) != hipSuccess) {
					dev_free(h, p);
					return GPUMT_E_HIP;
				}
				dev_free(h, h->scratch[0][s]);
			}
			h->scratch[0][s] = p;
			h->scratch_bytes[0][s] = need;
		}
	}
	if (h->trace >= 1)
		fprintf(stderr, "[gpumt brotli win] records %zu depth %u plane %zu fallback %d\n", nrec, win ? depth : 0u,
			win ? (size_t)4 * slice_in : (size_t)0, win ? 0 : 1);
	if (h->trace >= 1 && win && seg_log)
		fprintf(stderr, "[gpumt win chain] segments %zu seg_log %d heads %zu serial %d\n",
			pheads ? slice_rec * (((slice_in < chunk ? slice_in : chunk) + ((size_t)1 << seg_log) - 1) >> seg_log) : slice_rec,
			seg_log, pheads, par ? 0 : 1);
	if (!win)
		return gpumt_brotli_compress_batch_level(h, d_in, n, chunk, d_slots, slot_stride, d_rec_len, level, s);
	u32 *blk_len = (u32 *)h->scratch[0][s];
	u8 *seqbuf = (u8 *)h->scratch[0][s] + o_seq;
	u32 *heads = (u32 *)((u8 *)h->scratch[0][s] + o_head), *plane = (u32 *)((u8 *)h->scratch[0][s] + o_plane);
	PROF0(9);
	for (size_t r0 = 0; r0 < nrec; r0 += slice_rec) {
		const size_t nr = nrec - r0 < slice_rec ? nrec - r0 : slice_rec, i0 = r0 * chunk;
		const size_t ni = n - i0 < nr * chunk ? n - i0 : nr * chunk, nb = nr * bpr;
		const unsigned eg = (unsigned)(nb < egrid ? nb : egrid), cg = (unsigned)(nr < cgrid ? nr : cgrid);
		const u8 *in = (const u8 *)d_in + i0;
		u8 *slots = (u8 *)d_slots + r0 * slot_stride;
		const int rc = win_chain_launch(h, in, ni, chunk, nr, plane, heads, cg, par ? (u32 *)((u8 *)h->scratch[0][s] + need) : NULL,
						seg_log, s);
		if (rc)
			return rc;
		hipLaunchKernelGGL(zmt_brotli_enc_win_kernel, dim3(eg), dim3(64), 0, h->st[s], in, (u64)ni, (u32)chunk, (u32)nb, bpr,
				   slots, (u64)slot_stride, blk_len, seqbuf, (const u32 *)plane, depth);
		hipLaunchKernelGGL(zmt_brotli_assemble_kernel, dim3((unsigned)nr), dim3(256), 0, h->st[s], (u64)ni, (u32)chunk, (u32)nr,
				   bpr, slots, (u64)slot_stride, (const u32 *)blk_len, d_rec_len + r0);
	}
	PROF1(9);
	CK(hipGetLastError());
	return GPUMT_OK;
}

extern "C" const unsigned char zmt_brotli_static[], zmt_brotli_static_end[];

/* the record decoders: every record (only = 0xFFFFFFFF), or the records whose d_status is `only` on entry */
static int brotli_decompress_records(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off, const uint32_t *d_rec_len,
				     size_t nrec, void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
				     uint32_t *d_out_len, uint32_t *d_status, u32 only, int s);

int gpumt_brotli_decompress_batch(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
				  const uint32_t *d_rec_len, size_t nrec, void *d_out,
				  const uint64_t *d_out_off, const uint32_t *d_out_cap,
				  uint32_t *d_out_len, uint32_t *d_status, int s)
{
	return brotli_decompress_records(h, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len, d_status,
					 0xFFFFFFFFu, s);
}

static int brotli_decompress_records(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off, const uint32_t *d_rec_len,
				     size_t nrec, void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
				     uint32_t *d_out_len, uint32_t *d_status, u32 only, int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!h->d_brotli_static) {
		const size_t n = (size_t)(zmt_brotli_static_end - zmt_brotli_static);
		CK(hipMalloc(&h->d_brotli_static, n + 64));
		CK(hipMemcpy(h->d_brotli_static, zmt_brotli_static, n, hipMemcpyHostToDevice));
	}
	if (!h->bdec_waves) {
		int per_cu = 0;
		CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zmt_brotli_dec_kernel, 64, 0));
		h->bdec_waves = (per_cu > 0 ? per_cu : 4) * (h->num_cus > 0 ? h->num_cus : 256);
		if (getenv("GPUMT_VERBOSE"))
			fprintf(stderr, "gpumt: brotli decoder grid %d waves\n", h->bdec_waves);
	}
	const unsigned grid = (unsigned)(nrec < (size_t)h->bdec_waves ? nrec : (size_t)h->bdec_waves);
	if (want_scratch(h, 1, s, (size_t)grid * GPUMT_BROTLI_SCRATCH))
		return GPUMT_E_HIP;
	if (h->profile == 7 && !h->d_prof) {
		CK(hipMalloc((void **)&h->d_prof, 16 * sizeof(unsigned long long)));
		CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
	}
	PROF0(12);
	/* Two kernels.  zmt_brotli_dec4_kernel runs four records per wave (streams without context modelling / block
	 * switching; what it hands over -- status 102 -- goes to the general kernel): a quarter of the waves per record, each
	 * twice as slow as a one-record wave.  That wins as soon as the one-record kernel would need more than one round of
	 * its resident waves (8 192 records: 283 ms against 500), and loses below (1 024 records: 308 ms against 151), so
	 * the batch size chooses.  bdec_variant: 0 = that rule, 1 = the general kernel alone, 2 = dec4 first whatever the size */
	u32 want = only;
	const bool use4 = h->bdec_variant == 2 || (h->bdec_variant == 0 && nrec > (size_t)h->bdec_waves);
	if (use4 && h->profile != 7) {
		if (only == 0xFFFFFFFFu)
			hipLaunchKernelGGL(zmt_brotli_dec4_kernel, dim3((unsigned)((nrec + B4_NG - 1) / B4_NG)), dim3(64), 0, h->st[s],
					   (const u8 *)d_stream, d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off, d_out_cap,
					   d_out_len, d_status);
		else
			hipLaunchKernelGGL(zmt_brotli_dec4_wanted_kernel, dim3((unsigned)((nrec + B4_NG - 1) / B4_NG)), dim3(64), 0,
					   h->st[s], (const u8 *)d_stream, d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off,
					   d_out_cap, d_out_len, d_status, only);
		want = 102u;
	}
	if (h->profile == 7)
		hipLaunchKernelGGL(zmt_brotli_dec_kernel_prof, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_stream,
				   d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off, d_out_cap, d_out_len,
				   d_status, (u8 *)h->scratch[1][s], (const u8 *)h->d_brotli_static, want, h->d_prof);
	else
		hipLaunchKernelGGL(zmt_brotli_dec_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_stream,
				   d_rec_off, d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off, d_out_cap, d_out_len,
				   d_status, (u8 *)h->scratch[1][s], (const u8 *)h->d_brotli_static, want);
	PROF1(12);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* gpumt_lz4_decompress_batch_par's structure with the span stages of brotli_dec_rec.h in front of the record decoders */
int gpumt_brotli_decompress_batch_par(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off, const uint32_t *d_rec_len,
				      size_t nrec, void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
				      uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int s)
{
	static_assert(sizeof(BRec) == 32 && sizeof(B4Span) == 32, "record layout");
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	const hipStream_t st = h->st[s];
	if (d_rec_par)
		CK(hipMemsetAsync(d_rec_par, 0, nrec * 4, st));
	/* the stage's own areas.  Per record: the plan and the first span.  Per slice, sized once the plans are known: the span
	 * table and a status word per span */
	const size_t rec_bytes = (nrec * sizeof(BRec) + 255) & ~(size_t)255, word_bytes = (nrec * 4 + 255) & ~(size_t)255;
	const size_t need_a = rec_bytes + word_bytes;
	const size_t cap = h->brec_cap_mb ? (size_t)h->brec_cap_mb << 20 : ~(size_t)0;
	int par = h->brec_par, fallback = 0;
	if (par && ((h->brec_refused && need_a >= h->brec_refused) || need_a > cap ||
		    zrec_want(h, &h->brec_area[s], &h->brec_bytes[s], need_a, st))) {
		h->brec_refused = need_a;
		par = 0;
		fallback = 1;
	}
	if (par && rec_bytes > h->brec_pin_bytes[s]) {
		/* (the copy that read the old area was waited for by the call that queued it) */
		void *p = NULL;
		if (hipHostMalloc(&p, rec_bytes, hipHostMallocDefault) != hipSuccess || !p) {
			(void)hipGetLastError();
			h->brec_refused = need_a;
			par = 0;
			fallback = 1;
		} else {
			if (h->brec_pin[s])
				(void)hipHostFree(h->brec_pin[s]);
			h->brec_pin[s] = p;
			h->brec_pin_bytes[s] = rec_bytes;
		}
	}
	size_t npar = 0, nspans = 0, nslices = 0, max_span = 0, kept = 0;
	BRec *recs = (BRec *)h->brec_area[s];
	u32 *ufirst = par ? (u32 *)((u8 *)recs + rec_bytes) : NULL;
	const BRec *hrec = (const BRec *)h->brec_pin[s];
	const dim3 per_rec((unsigned)((nrec + 255) / 256)), tpb(256);
	BRecSlice S;
	if (par) {
		hipLaunchKernelGGL(zmt_brotli_rec_plan_kernel, per_rec, tpb, 0, st, (const u8 *)d_stream, d_rec_off, d_rec_len, (u32)nrec,
				   d_out_off, d_out_cap, (u32)h->brec_min_spans, recs);
		/* one round trip: the host sizes the span table and the launches of the execute stage from the plans */
		CK(hipMemcpyAsync(h->brec_pin[s], recs, nrec * sizeof(BRec), hipMemcpyDeviceToHost, st));
		CK(hipStreamSynchronize(st));
		for (size_t at = 0; brec_next_slice(hrec, nrec, at, BREC_SLICE_SPANS, &S); at = S.b) {
			nspans += S.nspan;
			nslices++;
			max_span = S.nspan > max_span ? S.nspan : max_span;
		}
		for (size_t i = 0; i < nrec; i++)
			npar += hrec[i].flags & BREC_ELIGIBLE;
		const size_t need_b = (max_span * (sizeof(B4Span) + 4) + 255) & ~(size_t)255, need = need_a + need_b;
		if (nslices && ((h->brec_refused && need >= h->brec_refused) || need > cap ||
				zrec_want(h, &h->brec_tab[s], &h->brec_tab_bytes[s], need_b, st))) {
			h->brec_refused = need;
			par = 0;
			fallback = 1;
		}
	}
	if (!par || !nslices) {
		/* nothing for the span stages (or no room for them): the serial call */
		if (h->trace >= 1)
			fprintf(stderr, "[gpumt brotli rec] records %zu par 0 spans 0 kept 0 fallback %d\n", nrec, fallback);
		return brotli_decompress_records(h, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len,
						 d_status, 0xFFFFFFFFu, s);
	}
	B4Span *spans = (B4Span *)h->brec_tab[s];
	u32 *span_st = (u32 *)(spans + max_span);
	/* every record is the record decoders' until finish says it was kept */
	CK(hipMemsetD32Async((hipDeviceptr_t)d_status, (int)BREC_TODO, nrec, st));
	for (size_t at = 0; brec_next_slice(hrec, nrec, at, BREC_SLICE_SPANS, &S); at = S.b) {
		const u32 n = (u32)(S.b - S.a);
		const dim3 per_slice((n + 255) / 256);
		hipLaunchKernelGGL(zmt_brotli_rec_scan_kernel, dim3(1), tpb, 0, st, (const BRec *)(recs + S.a), n, ufirst + S.a);
		hipLaunchKernelGGL(zmt_brotli_rec_table_kernel, per_slice, tpb, 0, st, (const u8 *)d_stream, (const BRec *)(recs + S.a), n,
				   (u32)S.a, (const u32 *)(ufirst + S.a), S.nspan, spans);
		hipLaunchKernelGGL(zmt_brotli_dec4_span_kernel, dim3((S.nspan + B4_NG - 1) / B4_NG), dim3(64), 0, st, (const u8 *)d_stream,
				   (const B4Span *)spans, S.nspan, (u8 *)d_out, span_st);
		hipLaunchKernelGGL(zmt_brotli_rec_finish_kernel, per_slice, tpb, 0, st, (const BRec *)(recs + S.a), n,
				   (const u32 *)(ufirst + S.a), S.nspan, (const B4Span *)spans, (const u32 *)span_st, d_out_len + S.a,
				   d_status + S.a,
				   d_rec_par ? d_rec_par + S.a : (u32 *)NULL);
	}
	CK(hipGetLastError());
	if (h->trace >= 1) {
		/* (the count of kept records costs a round trip: the trace alone pays it) */
		u32 *hst = (u32 *)malloc(nrec * 4);
		if (hst && hipMemcpyAsync(hst, d_status, nrec * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
		    hipStreamSynchronize(st) == hipSuccess)
			for (size_t i = 0; i < nrec; i++)
				kept += hst[i] == GPUMT_ST_OK;
		free(hst);
		fprintf(stderr, "[gpumt brotli rec] records %zu par %zu spans %zu kept %zu fallback 0\n", nrec, npar, nspans, kept);
	}
	/* everything the span stages did not keep is decoded and judged by the record decoders */
	return brotli_decompress_records(h, d_stream, d_rec_off, d_rec_len, nrec, d_out, d_out_off, d_out_cap, d_out_len, d_status,
					 BREC_TODO, s);
}

/* ---- snappy-mt (snappy.hip): persistent waves, one record at a time ---- */
size_t gpumt_snappy_slot_stride(size_t chunk)
{
	return (16 + 32 + chunk + chunk / 6 + 255) & ~(size_t)255; /* header + snappy_max_compressed_length */
}

static int snappy_waves(gpumt_ctx *h, int *cache, const void *kernel, const char *what)
{
	if (!*cache) {
		int per_cu = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess)
			per_cu = 0;
		*cache = (per_cu > 0 ? per_cu : 8) * (h->num_cus > 0 ? h->num_cus : 256);
		if (getenv("GPUMT_VERBOSE"))
			fprintf(stderr, "gpumt: snappy %s grid %d waves\n", what, *cache);
	}
	return *cache;
}

int gpumt_snappy_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				size_t slot_stride, uint32_t *d_rec_len, int s)
{
	if (!h || !STREAM_OK(s) || chunk == 0 || chunk > 0x40000000u || slot_stride < gpumt_snappy_slot_stride(chunk))
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	const size_t nrec = gpumt_lz4_record_count(n, chunk);
	if (nrec > 0x7FFFFFFFu)
		return GPUMT_E_ARG;
	const int waves = snappy_waves(h, &h->senc_waves, (const void *)zmt_snappy_enc_kernel, "encoder");
	const unsigned grid = (unsigned)(nrec < (size_t)waves ? nrec : (size_t)waves);
	hipLaunchKernelGGL(zmt_snappy_enc_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_in, (u64)n,
			   (u32)chunk, (u32)nrec, (u8 *)d_slots, (u64)slot_stride, d_rec_len);
	CK(hipGetLastError());
	return GPUMT_OK;
}

int gpumt_snappy_decompress_batch(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
				  const uint32_t *d_rec_len, size_t nrec, void *d_out,
				  const uint64_t *d_out_off, const uint32_t *d_out_cap,
				  uint32_t *d_out_len, uint32_t *d_status, int s)
{
	if (!h || !STREAM_OK(s) || nrec == 0 || nrec > 0x3FFFFFFFu)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (h->sdec_variant == 1) {
		const int waves = snappy_waves(h, &h->sdec2_waves, (const void *)zmt_snappy_dec2_kernel, "decoder (batched)");
		const unsigned grid = (unsigned)(nrec < (size_t)waves ? nrec : (size_t)waves);
		hipLaunchKernelGGL(zmt_snappy_dec2_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_stream, d_rec_off,
				   d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off, d_out_cap, d_out_len, d_status);
		CK(hipGetLastError());
		return GPUMT_OK;
	}
	const int waves = snappy_waves(h, &h->sdec_waves, (const void *)zmt_snappy_dec_kernel, "decoder");
	const unsigned grid = (unsigned)(nrec < (size_t)waves ? nrec : (size_t)waves);
	hipLaunchKernelGGL(zmt_snappy_dec_kernel, dim3(grid), dim3(64), 0, h->st[s], (const u8 *)d_stream, d_rec_off,
			   d_rec_len, (u32)nrec, (u8 *)d_out, d_out_off, d_out_cap, d_out_len, d_status);
	CK(hipGetLastError());
	return GPUMT_OK;
}

/* read (and clear) the phase counters of the profiling decoder; returns count written */
int gpumt_debug_counters(gpumt_ctx *h, unsigned long long *dst, int n)
{
	if (!h || !dst || n < 16)
		return GPUMT_E_ARG;
	if (use(h))
		return GPUMT_E_HIP;
	if (!h->d_prof) {
		CK(hipMalloc((void **)&h->d_prof, 16 * sizeof(unsigned long long)));
		CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
	}
	CK(hipDeviceSynchronize());
	CK(hipMemcpy(dst, h->d_prof, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	CK(hipMemset(h->d_prof, 0, 16 * sizeof(unsigned long long)));
	return 16;
}

int gpumt_set_variant(gpumt_ctx *h, const char *what, int variant)
{
	int prev = -1;
	if (!h || !what)
		return -1;
	if (!strcmp(what, "lz4_dec")) {
		prev = h->dec_variant;
		h->dec_variant = variant;
	} else if (!strcmp(what, "lz4_ring")) {
		prev = h->lz4_ring;
		h->lz4_ring = variant;
	} else if (!strcmp(what, "lz4_enc")) {
		prev = h->enc_variant;
		h->enc_variant = variant;
	} else if (!strcmp(what, "lz4_dec_pad")) {
		prev = h->dec_pad;
		h->dec_pad = variant;
	} else if (!strcmp(what, "brotli_dec")) {
		prev = h->bdec_variant;
		h->bdec_variant = variant;
	} else if (!strcmp(what, "debug_free")) {
		prev = h->debug_free;
		h->debug_free = variant;
	} else if (!strcmp(what, "k2x")) {
		prev = h->xflags;
		h->xflags = variant;
	} else if (!strcmp(what, "hc_waves")) {
		prev = h->hc_waves;
		h->hc_waves = variant;
	} else if (!strcmp(what, "zstd_dec")) {
		prev = h->zdec_variant;
		h->zdec_variant = variant;
	} else if (!strcmp(what, "zstd_seq")) {
		prev = h->zseq_variant;
		h->zseq_variant = variant;
	} else if (!strcmp(what, "zstd_run_pre")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->zrun_pre;
		h->zrun_pre = variant;
	} else if (!strcmp(what, "zstd_run_par")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->zrun_par;
		h->zrun_par = variant;
	} else if (!strcmp(what, "zstd_rec_par")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->zrec_par;
		h->zrec_par = variant;
	} else if (!strcmp(what, "zstd_rec_min_blocks")) {
		if (variant < 1 || variant > 65536)
			return -1;
		prev = h->zrec_min_blocks;
		h->zrec_min_blocks = variant;
	} else if (!strcmp(what, "zstd_rec_slice_blocks")) {
		if (variant < 2 || variant > 65536)
			return -1;
		prev = h->zrec_slice_blocks;
		h->zrec_slice_blocks = variant;
	} else if (!strcmp(what, "zstd_rec_cap_mb")) {
		if (variant < 0)
			return -1;
		prev = h->zrec_cap_mb;
		h->zrec_cap_mb = variant;
		h->zrec_refused = 0; /* (a new cap: ask again) */
	} else if (!strcmp(what, "zstd_win_depth")) {
		if (variant < 0 || variant > 256)
			return -1;
		prev = h->zwin_depth;
		h->zwin_depth = variant;
	} else if (!strcmp(what, "zstd_win_cap_mb")) {
		if (variant < 0)
			return -1;
		prev = h->zwin_cap_mb;
		h->zwin_cap_mb = variant;
		h->zwin_refused = 0; /* (a new cap: ask again) */
	} else if (!strcmp(what, "brotli_win_depth")) {
		if (variant < 0 || variant > 256)
			return -1;
		prev = h->bwin_depth;
		h->bwin_depth = variant;
	} else if (!strcmp(what, "brotli_win_cap_mb")) {
		if (variant < 0)
			return -1;
		prev = h->bwin_cap_mb;
		h->bwin_cap_mb = variant;
		h->bwin_refused = 0; /* (a new cap: ask again) */
	} else if (!strcmp(what, "win_chain_par")) {
		if (variant != 0 && variant != 1 && (variant < 12 || variant > 24))
			return -1;
		prev = h->wchain_par;
		h->wchain_par = variant;
	} else if (!strcmp(what, "win_chain_cap_mb")) {
		if (variant < 0)
			return -1;
		prev = h->wchain_cap_mb;
		h->wchain_cap_mb = variant;
		h->wchain_refused = 0; /* (a new cap: ask again) */
	} else if (!strcmp(what, "lz4_run_par")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->lrun_par;
		h->lrun_par = variant;
	} else if (!strcmp(what, "lz4_block_seg")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->lblk_seg;
		h->lblk_seg = variant;
	} else if (!strcmp(what, "lz4_seg_bytes")) {
		if (variant < 256 || variant > (4 << 20) || (variant & (variant - 1)))
			return -1;
		prev = h->lseg_bytes;
		h->lseg_bytes = variant;
	} else if (!strcmp(what, "lz4_rec_par")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->lrec_par;
		h->lrec_par = variant;
	} else if (!strcmp(what, "lz4_rec_seg")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->lrec_seg;
		h->lrec_seg = variant;
	} else if (!strcmp(what, "lz4_rec_min_blocks")) {
		if (variant < 2 || variant > 65536)
			return -1;
		prev = h->lrec_min_blocks;
		h->lrec_min_blocks = variant;
	} else if (!strcmp(what, "lz4_rec_slice_blocks")) {
		if (variant < 2 || variant > 65536)
			return -1;
		prev = h->lrec_slice_blocks;
		h->lrec_slice_blocks = variant;
	} else if (!strcmp(what, "lz4_rec_cap_mb")) {
		if (variant < 0)
			return -1;
		prev = h->lrec_cap_mb;
		h->lrec_cap_mb = variant;
		h->lrec_refused = 0; /* (a new cap: ask again) */
	} else if (!strcmp(what, "brotli_rec_par")) {
		if (variant != 0 && variant != 1)
			return -1;
		prev = h->brec_par;
		h->brec_par = variant;
	} else if (!strcmp(what, "brotli_rec_min_spans")) {
		if (variant < 2 || variant > 65536)
			return -1;
		prev = h->brec_min_spans;
		h->brec_min_spans = variant;
	} else if (!strcmp(what, "brotli_rec_cap_mb")) {
		if (variant < 0)
			return -1;
		prev = h->brec_cap_mb;
		h->brec_cap_mb = variant;
		h->brec_refused = 0; /* (a new cap: ask again) */
	} else if (!strcmp(what, "snappy_dec")) {
		prev = h->sdec_variant;
		h->sdec_variant = variant;
	} else if (!strcmp(what, "profile")) {
		prev = h->profile;
		h->profile = variant;
	}
	return prev;
}

} /* extern "C" */
