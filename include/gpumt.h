/*
 * gpumt.h -- C ABI of the MI355X device engine that replaces zstdmt's per-chunk codec dispatch.
 *
 * This is the *internal* boundary the reference does not have (last row):
 * the host library behind LZ4MT_* (include/lz4-mt.h) hands batches of chunks / records to the GPU
 * through these calls, exactly where the reference's worker threads call into liblz4:
 *
 *   gpumt_lz4_compress_batch   replaces  LZ4F_compressFrame    @ lib/lz4-mt_compress.c:281  (C2)
 *   gpumt_lz4_compress_batch_level  the same call with prefs.compressionLevel >= 3 (HC, :141-146)
 *                                        + header emit          @ lib/lz4-mt_compress.c:294-298 (F5)
 *   gpumt_lz4_slot_stride      replaces  LZ4F_compressFrameBound@ lib/lz4-mt_compress.c:232,244 (C1)
 *   gpumt_lz4_compact          replaces  pt_write ordering      @ lib/lz4-mt_compress.c:178-205 (F4)
 *   gpumt_lz4_decompress_batch replaces  LZ4F_decompress        @ lib/lz4-mt_decompress.c:349-362 (C3)
 *                                        + size probe           @ lib/lz4-mt_decompress.c:329-334 (F10)
 *   gpumt_lz4_decompress_blocks replaces the streaming LZ4F_decompress @ lib/lz4-mt_decompress.c:391-483 (plain .lz4)
 *   gpumt_zstd_decompress_blocks replaces the streaming ZSTD_decompressStream @ lib/zstd-mt_decompress.c:552-687 (plain .zst)
 *
 * Plain C types only: opaque handle, device pointers as void*, sizes as integers.  Nothing here
 * falls back to the CPU: every entry point returns GPUMT_E_NODEVICE/E_HIP when the HIP runtime or
 * the gfx950 device is unavailable.
 *
 * All device pointers must come from gpumt_malloc() of the same handle (or any allocation of the
 * same HIP device).  "stream" arguments are small integers 0..GPUMT_NSTREAMS-1 naming the
 * handle's own HIP streams (0 = compute, 1 = H2D, 2 = D2H in the host pipeline).
 */
#ifndef GPUMT_H
#define GPUMT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* streams 0..3: kernels / H2D / small D2H / bulk D2H of the host engines' pipeline; 4..11: one extra
 * kernel stream per batch slot, so that the batches of a pipeline overlap on the device (every
 * launching stream has its own internal scratch) */
#define GPUMT_NSTREAMS 16

enum {
	GPUMT_OK = 0,
	GPUMT_E_NODEVICE = -1, /* no HIP device / runtime */
	GPUMT_E_HIP = -2,      /* a HIP call failed; see gpumt_last_error() */
	GPUMT_E_ARG = -3,
	GPUMT_E_NOMEM = -4
};

/* per-record status words written by gpumt_lz4_decompress_batch (0 = frame decoded and verified) */
enum {
	GPUMT_ST_OK = 0,
	GPUMT_ST_BAD_RECORD = 1,   /* skippable header wrong (magic / len != 4 / csize)      -> data_error  */
	GPUMT_ST_BAD_FRAME = 2,    /* LZ4F magic / version / reserved bits / header checksum -> compression_library */
	GPUMT_ST_BAD_BLOCK = 3,    /* malformed block (overrun, zero offset, offset too far)  */
	GPUMT_ST_SIZE_MISMATCH = 4,/* decoded bytes != content-size field                     */
	GPUMT_ST_BAD_CHECKSUM = 5, /* XXH32 content checksum mismatch                         */
	GPUMT_ST_TRAILING = 6,     /* record longer than the frame it carries -> frame_decompress */
	GPUMT_ST_UNSUPPORTED = 7   /* valid LZ4F feature the device path does not decode (block checksum, dictID) */
};

typedef struct gpumt_ctx gpumt_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
int  gpumt_device_count(void);
/* device: HIP device index, or GPUMT_DEVICE_DEFAULT = the index in the environment variable
 * GPUMT_DEVICE (0 when unset) -- what the LZ4MT_* / ZSTDCB_* / BROTLIMT_* contexts use */
#define GPUMT_DEVICE_DEFAULT (-1)
int  gpumt_open(int device, gpumt_ctx **out);
void gpumt_close(gpumt_ctx *h);
const char *gpumt_last_error(gpumt_ctx *h);
const char *gpumt_device_name(gpumt_ctx *h);
/* NUMA node of the host the device's PCIe function hangs off (sysfs numa_node), -1 when the host does not say.  Pinned
 * memory from gpumt_host_alloc lives on that node: a host thread that fills or drains it copies 25-30 % faster from
 * there (profiles/r06_sweeps/api_numa.txt), which is why the host engines' reader / writer threads bind themselves to it */
int gpumt_host_node(gpumt_ctx *h);

/* ---- memory / transfers / sync ------------------------------------------------------------ */
/* Freed buffers go to process-wide caches (device: GPUMT_DEVICE_CACHE_MB, pinned host:
 * GPUMT_PINNED_CACHE_MB, 16384 each by default; 0 disables) and from there to the next allocation of a
 * similar size, without a device-wide wait: free a buffer only when no queued work uses it. */
/* Debug guard for that contract: with GPUMT_DEBUG_FREE=1 in the environment (or gpumt_set_variant(h, "debug_free", 1))
 * gpumt_free / gpumt_host_free first ask every stream of the context whether work is still queued; if so they count the
 * call (gpumt_debug_free_busy), report it on stderr and wait for the streams before the buffer is recycled. */
void *gpumt_malloc(gpumt_ctx *h, size_t bytes);
void  gpumt_free(gpumt_ctx *h, void *dptr);
void *gpumt_host_alloc(gpumt_ctx *h, size_t bytes);          /* pinned */
void  gpumt_host_free(gpumt_ctx *h, void *hptr);
/* Pin / unpin memory the caller owns (hipHostRegister): an application buffer, or one mapping shared by the ranks
 * of a multi-GPU job into which every GPU copies its segment at its offset (bench.py --gather d2h). */
int gpumt_host_register(gpumt_ctx *h, void *p, size_t bytes);
int gpumt_host_unregister(gpumt_ctx *h, void *p);
/* Freed device and pinned buffers stay in process-wide caches (GPUMT_DEVICE_CACHE_MB / GPUMT_PINNED_CACHE_MB, 16 GiB
 * each by default) for the next context; this releases whatever is idle and returns the bytes given back. */
size_t gpumt_trim_caches(gpumt_ctx *h);
/* calls of gpumt_free / gpumt_host_free the debug guard caught with work queued, process-wide, since the last call */
unsigned long gpumt_debug_free_busy(void);
int   gpumt_memcpy_h2d(gpumt_ctx *h, void *dst, const void *src, size_t n, int stream);
int   gpumt_memcpy_d2h(gpumt_ctx *h, void *dst, const void *src, size_t n, int stream);
int   gpumt_memcpy_d2d(gpumt_ctx *h, void *dst, const void *src, size_t n, int stream);
/* Device -> pinned host memory (from gpumt_host_alloc) by a kernel on `stream`: min(n, *d_n) bytes when
 * d_n (a uint64 in device memory, e.g. the total gpumt_lz4_compact leaves at d_rec_off[nrec]) is
 * given, else n.  Both addresses 16-byte aligned.  What the host engines use for results: the size
 * stays on the device and batches on different streams overlap (see pack.hip). */
int   gpumt_push_host(gpumt_ctx *h, void *dst_host, const void *src, size_t n, const uint64_t *d_n, int stream);
int   gpumt_memset(gpumt_ctx *h, void *dst, int byte, size_t n, int stream);
int   gpumt_stream_sync(gpumt_ctx *h, int stream);
int   gpumt_device_sync(gpumt_ctx *h);
/* make `waiter` wait (on device) for everything queued so far on `signaler` */
int   gpumt_stream_wait(gpumt_ctx *h, int waiter, int signaler);
/* Markers: gpumt_mark(id, stream) records marker id (0..GPUMT_NMARKS-1) behind everything queued so
 * far on `stream`; gpumt_mark_sync(id) blocks the calling host thread until that point is reached
 * (and nothing queued later).  Thread-safe: one thread may wait on a marker while another queues
 * work. */
#define GPUMT_NMARKS 16
int   gpumt_mark(gpumt_ctx *h, int id, int stream);
int   gpumt_mark_sync(gpumt_ctx *h, int id);
/* raw hipStream_t of a stream index, for callers that interoperate (e.g. RCCL via torch) */
void *gpumt_stream_handle(gpumt_ctx *h, int stream);

/* ---- HIP-event timing on the handle's streams (bench.py's roofline leg) -------------------- */
int   gpumt_timer_start(gpumt_ctx *h, int slot, int stream);   /* slot 0..15 */
int   gpumt_timer_stop(gpumt_ctx *h, int slot, int stream);
int   gpumt_timer_ms(gpumt_ctx *h, int slot, float *ms);       /* syncs on the stop event */

/* ---- LZ4 (lz4-mt level 1..2 = LZ4 "fast", acceleration 1) ---------------------------------- */

/* Bytes one record can occupy: 12 + LZ4F_compressFrameBound(chunk), rounded up to 256. */
size_t gpumt_lz4_slot_stride(size_t chunk);

/* Number of records the reference emits for n input bytes (>= 1: empty input -> one empty frame). */
size_t gpumt_lz4_record_count(size_t n, size_t chunk);

/*
 * Compress d_in[0..n) as consecutive chunks of `chunk` bytes (last one ragged).  Record i
 * (12-byte skippable header + one LZ4 frame, byte-identical to the reference's output for that
 * chunk) is written at d_slots + i*slot_stride and its length to d_rec_len[i].
 * Uses internal scratch of 4 bytes per chunk for the XXH32 content checksums.
 */
int gpumt_lz4_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk,
			     void *d_slots, size_t slot_stride, uint32_t *d_rec_len, int stream);

/*
 * The same with lz4-mt's compression level (prefs.compressionLevel, lib/lz4-mt_compress.c:141-146):
 * 1..2 = LZ4 fast (what gpumt_lz4_compress_batch does), 3..9 = LZ4 HC hash-chain parser with
 * 4..256 searches per position (liblz4 1.9.3 lz4hc.c; level 9 with its pattern analysis), 10..12 =
 * the LZ4 HC optimal parser (96 / 512 / 16 384 searches): byte-identical to the reference at that
 * level, and slower with every level (a chain link is a dependent memory access).
 * HC keeps a 320 KiB table set per wave in internal scratch (at most GPUMT_LZ4HC_WAVES of them).
 */
#define GPUMT_LZ4HC_SCRATCH 327936u
#define GPUMT_LZ4HC_WAVES 4096u
int gpumt_lz4_level_supported(int level);
int gpumt_lz4_compress_batch_level(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk,
				   void *d_slots, size_t slot_stride, uint32_t *d_rec_len, int level,
				   int stream);

/*
 * Ordered concatenation: d_rec_off[i] = sum of d_rec_len[0..i), d_rec_off[nrec] = total, and the
 * records are packed into d_stream at those offsets (the MT stream, ready for fn_write / D2H).
 */
int gpumt_lz4_compact(gpumt_ctx *h, const void *d_slots, size_t slot_stride,
		      const uint32_t *d_rec_len, size_t nrec, void *d_stream,
		      uint64_t *d_rec_off, int stream);

/*
 * For records located at d_stream + d_rec_off[i] (length d_rec_len[i], including the 12-byte
 * skippable header) read each frame's content-size field and produce d_out_len[i] and the
 * exclusive scan d_out_off[0..nrec] (what pt_decompress does per record at :333-334).
 */
int gpumt_lz4_probe_sizes(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
			  const uint32_t *d_rec_len, size_t nrec, uint32_t *d_out_len,
			  uint64_t *d_out_off, int stream);

/*
 * Decode nrec records.  Record i's content goes to d_out + d_out_off[i] and must be exactly
 * d_out_len[i] bytes; header, block structure, content size and XXH32 content checksum are
 * verified.  d_status[i] receives a GPUMT_ST_* code.
 * stream_bytes / out_bytes: upper bounds of the bytes spanned by the records in d_stream and by
 * their contents in d_out (they size the internal token-list scratch, about 0.7 x stream_bytes).
 * The d_stream allocation must extend at least 256 readable bytes past stream_bytes: the parse
 * kernel fetches whole aligned 128-byte lines (their contents past the last record are ignored).
 */
int gpumt_lz4_decompress_batch(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
			       const uint64_t *d_rec_off, const uint32_t *d_rec_len, size_t nrec,
			       void *d_out, size_t out_bytes, const uint64_t *d_out_off,
			       uint32_t *d_out_len, uint32_t *d_status, int stream);

/*
 * gpumt_lz4_decompress_batch with the records of several linked blocks decoded block-parallel (opt-in; what
 * GPUMT_LZ4_REC_PAR=1 makes LZ4MT_decompressDCtx call).  Same arguments and slack rule, and for every record the same
 * status and d_out_len; for every record whose status is GPUMT_ST_OK the same output bytes (the output range of a record
 * that fails is unspecified, as in the block calls), and nothing outside a record's [d_out_off[i], d_out_off[i] +
 * d_out_len[i]) is written.  d_rec_par (nrec words, may be NULL) receives per record the number of its blocks whose result
 * came from the block call on the tables made here and was kept, 0 for every other record.  A return value other than
 * GPUMT_OK (a launch failed) leaves the batch undefined.
 * The stages, stream-ordered, none of which waits on another wave (lz4_dec_rec.h; the LZ4 twin of
 * gpumt_zstd_decompress_batch_par below):
 *   count   one lane per record checks the 12-byte header and the LZ4F frame header (magic, version, reserved bits, BD,
 *           content size, dictID, header checksum) and hops from block header to block header to the end mark.  A record is
 *           eligible when both headers are well formed, the blocks are linked, the stated content size equals d_out_len[i],
 *           is not 0 and at most 0xFFFE0000, every block lies inside the record with a size of at most the frame's block
 *           maximum, the end mark is there, exactly the promised 4 checksum bytes (or none) follow it, and the record has
 *           lz4_rec_min_blocks .. 65536 parts: blocks, or on the seg route max(blocks, ceil(content / lz4_seg_bytes)).
 *           Block checksums, a dictID and block maxima above 64 KiB are eligible; frames of independent blocks and frames
 *           without a content size are not.  The stage decides no verdict.
 *   (host)  one copy of the counts to pinned memory and one hipStreamSynchronize of `stream`: the host cuts the batch into
 *           slices of consecutive records with at most 4096 eligible records, lz4_rec_slice_blocks blocks (a record of
 *           more is a slice of its own) and 0xFFFFFFF0 stream bytes.  A slice passes d_stream and d_out offset to its first
 *           eligible record (rounded down to 256), so the origin plane of the block call is 2 x the slice's output span.
 *   table   per slice a scan of the block counts, then one lane per eligible record writes its gpumt_lz4_block entries
 *           (stored flag, block checksum word, blkmax) and one gpumt_lz4_run (low = out_off, out_cap = the content size).
 *   blocks  gpumt_lz4_decompress_blocks_par, or gpumt_lz4_decompress_blocks_seg with the handle's lz4_seg_bytes, on the
 *           slice's tables, unchanged: either falls back by its own rules.
 *   finish  one lane per eligible record keeps it when the run's status is OK and its length is the stated content size.
 *           A kept record gets d_rec_par, its content checksum words, and a mark in a scratch status word.
 *   records the record decoders of gpumt_lz4_decompress_batch over the whole batch with those words as their "kept" array:
 *           a kept record is passed by, every other record is decoded and judged there, so the verdicts are the serial
 *           call's by construction.  A merge writes GPUMT_ST_OK for the kept records and the XXH32 verify runs once over
 *           all records.
 * Internal scratch: areas of its own, which the block calls and the record decoders do not replace -- 76 bytes per record
 * and, for the largest slice, 32 bytes per block and 40 per eligible record -- next to theirs.  If the device refuses them,
 * or they exceed lz4_rec_cap_mb, the call is gpumt_lz4_decompress_batch (d_rec_par 0) and that size is not asked for again.
 * gpumt_set_variant: "lz4_rec_par" 1 = default, 0 = the record decoders alone; "lz4_rec_seg" 0 = blocks_par (default), 1 =
 * blocks_seg (GPUMT_LZ4_REC_SEG); "lz4_rec_min_blocks" 2..65536 (default 4096, from profiles/lz4_rec_par.txt: records of
 * 64 KiB blocks decode faster through the record decoders up to 1024 blocks per record, records the record decoders give to
 * one wave each -- block checksums, a dictID, blocks above 64 KiB -- decode 2 to 8 times faster through this call from 4
 * blocks on, so set 4 for those; GPUMT_LZ4_REC_MIN_BLOCKS); "lz4_rec_slice_blocks" 2..65536 (default 4096; GPUMT_LZ4_REC_SLICE_BLOCKS); "lz4_rec_cap_mb"
 * (0 = none).  Values out of range are refused with -1 and change nothing.  With GPUMT_TRACE=1 every call prints
 * `[gpumt lz4 rec] records N par P blocks B slices S fallback F route seg|par` (P eligible records with B blocks in S calls
 * of the block stages; F = 1: this stage's own scratch was refused and the record decoders took the whole batch).
 */
int gpumt_lz4_decompress_batch_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				   const uint64_t *d_rec_off, const uint32_t *d_rec_len, size_t nrec,
				   void *d_out, size_t out_bytes, const uint64_t *d_out_off,
				   uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int stream);

/*
 * Block-level LZ4 decode: what the plain .lz4 path of LZ4MT_decompressDCtx uses in place of one record per frame
 * (replaces the streaming LZ4F_decompress of st_decompress, lib/lz4-mt_decompress.c:391-483).  The caller walks the
 * frame and block headers and passes a table of blocks and a list of runs; one wave decodes a run, its blocks back to
 * back from d_out + out_off, at most out_cap bytes.
 *   independent-block frame: every block is its own run, low = out_off, out_cap = what the block can decode to
 *                            (min(blkmax, 255 x src_len), or src_len when stored); the slots are packed afterwards
 *                            (gpumt_lz4_pack_runs) unless every one came out full
 *   linked-block frame:      one run holds the frame's blocks of this batch; low reaches back over the history (the
 *                            last min(64 KiB, bytes so far) of the frame's output) that the caller copied in front
 *                            of out_off, so out_off - low <= 65536
 * d_block_len[b] receives block b's decoded length, d_run_len[r] the run's, d_status[r] GPUMT_ST_OK, GPUMT_ST_BAD_BLOCK
 * (malformed block, block above blkmax or above the room left; liblz4's end-of-block rules are measured from blkmax),
 * GPUMT_ST_BAD_CHECKSUM (block checksum) or GPUMT_ST_BAD_RECORD (a table entry that leaves stream_bytes / out_bytes:
 * the tables are device memory, the kernel checks them).  After an error the run's later blocks are not decoded.
 * Frame header, end mark, content size and content checksum are the caller's (gpumt_xxh32_carry).  No d_stream slack.
 */
#define GPUMT_LZ4B_STORED 1u   /* the block body is the content */
#define GPUMT_LZ4B_CHECKSUM 2u /* `checksum` is the XXH32 of the block body */
typedef struct {
	uint64_t src_off; /* block body in d_stream */
	uint32_t src_len;
	uint32_t flags;
	uint32_t blkmax;  /* the frame's block maximum, 64 KiB .. 4 MiB */
	uint32_t checksum;
} gpumt_lz4_block;
typedef struct {
	uint64_t low;     /* lowest byte of d_out a match of this run may read */
	uint64_t out_off;
	uint32_t out_cap; /* at most 0xFFFE0000: positions inside a run are 32 bits */
	uint32_t first, count; /* blocks [first, first + count) */
	uint32_t reserved;
} gpumt_lz4_run;
#define GPUMT_LZ4_BLOCKS_MAX 0x00FFFFFFu
int gpumt_lz4_decompress_blocks(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				const gpumt_lz4_block *d_blocks, size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun,
				void *d_out, size_t out_bytes, uint32_t *d_block_len, uint32_t *d_run_len,
				uint32_t *d_status, int stream);
/*
 * The same call with the blocks of a linked run decoded side by side: same arguments, tables, statuses, d_block_len and
 * d_run_len as gpumt_lz4_decompress_blocks (after an error in block k: the run's length is the sum of the blocks before k,
 * d_block_len[k..] is not written, the status is that of the first failing block in block order; the bytes of d_out in
 * [out_off + run_len, out_off + out_cap) are unspecified, nothing outside [out_off, out_off + out_cap) is written).
 * Runs of one block -- every run of an independent-block frame -- are decoded by the same code as there.  Runs of two or
 * more blocks take five stream-ordered launches, none of which waits on another wave: a plan (one wave), one wave per block
 * that checks the table entry and the block checksum and walks the tokens without copying (decoded length, every verdict
 * that does not depend on history), one wave per run that turns lengths into positions and finds the first failing block,
 * one wave per block that decodes the block at its final position -- a match source below the block's first byte is not
 * read; its distance before the block's start, 1..65535, goes into a u16 plane, one entry per output byte, and is copied
 * along with the value by matches inside the block -- and one workgroup per run that fills those bytes in, block after
 * block.  The runs of two or more blocks must name ascending, disjoint block ranges in run order (a linked frame's blocks
 * in a batch are such a run); any other table is decoded by the serial code, with the same results.
 * Internal scratch: GPUMT_LZ4_PAR_SCRATCH(out_bytes) + 20 bytes per block; when the device cannot provide it the call
 * decodes serially rather than fail, keeps the scratch it has, and does not ask for that size again.
 * GPUMT_LZ4_RUN_PAR=0 in the environment or gpumt_set_variant(h, "lz4_run_par", 0) make the call
 * gpumt_lz4_decompress_blocks (1 turns it on again; other values are refused).
 */
#define GPUMT_LZ4_PAR_SCRATCH(out_bytes) (2 * (size_t)(out_bytes) + 8)
int gpumt_lz4_decompress_blocks_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				    const gpumt_lz4_block *d_blocks, size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun,
				    void *d_out, size_t out_bytes, uint32_t *d_block_len, uint32_t *d_run_len,
				    uint32_t *d_status, int stream);
/*
 * The same call with every block cut into segments that are decoded side by side: same arguments, tables, statuses,
 * d_block_len, d_run_len and error contract as gpumt_lz4_decompress_blocks_par, for linked runs and for independent blocks
 * (runs of one block) alike.  A segment is a stretch of one block's sequences that starts at a token: the first one whose
 * output position is at or behind k x seg_bytes (a stored block is cut at k x seg_bytes), so a block has at most
 * ceil(decoded length / seg_bytes) segments and a sequence longer than a segment stays whole.  The five launches of
 * gpumt_lz4_decompress_blocks_par with that unit: the plan also gives every block room for its cuts, the wave that measures
 * a block writes the cuts (input and output position, block-relative) down, one wave per segment decodes it at its final
 * position -- origins are distances before the segment's start; the end-of-block rules and the history check see the
 * block's and the run's positions as the serial decoder does -- and one workgroup per run fills the origins in, segment
 * after segment.  No wave waits on another wave of its launch.  Every run of one block or more must name ascending,
 * disjoint block ranges in run order and the runs' areas must not overlap; any other table is decoded by the serial code.
 * d_block_seg[b] receives the number of segments block b was executed in, for the blocks in front of a run's first failing
 * one; 0 for every other block and wherever the serial code decoded: the table refused, the scratch refused, or a run of
 * one block that is no longer than a segment.
 * gpumt_set_variant(h, "lz4_seg_bytes", n) sets seg_bytes: a power of two, 256 .. 4 MiB, 65536 by default; anything else
 * is refused with -1 and changes nothing.  GPUMT_LZ4_BLOCK_SEG=0 in the environment or
 * gpumt_set_variant(h, "lz4_block_seg", 0) make the call gpumt_lz4_decompress_blocks (1 turns it on again; other values are
 * refused).  Internal scratch: GPUMT_LZ4_SEG_SCRATCH(out_bytes, nblk, seg_bytes) -- the origin plane, which is the cached
 * allocation of gpumt_lz4_decompress_blocks_par, 12 bytes per possible cut (out_bytes / seg_bytes + nblk: the cut and its
 * segment's word) and 32 bytes per block; when the device cannot provide it the call decodes serially rather than fail,
 * keeps the scratch it has, does not ask for that size again, and d_block_seg is 0.
 */
#define GPUMT_LZ4_SEG_SCRATCH(out_bytes, nblk, seg_bytes) \
	(GPUMT_LZ4_PAR_SCRATCH(out_bytes) + 12 * ((size_t)(out_bytes) / (size_t)(seg_bytes) + (size_t)(nblk)) + 32 * (size_t)(nblk) + 256)
int gpumt_lz4_decompress_blocks_seg(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				    const gpumt_lz4_block *d_blocks, size_t nblk, const gpumt_lz4_run *d_runs, size_t nrun,
				    void *d_out, size_t out_bytes, uint32_t *d_block_len, uint32_t *d_run_len,
				    uint32_t *d_status, uint32_t *d_block_seg, int stream);
/* Ordered concatenation of what the runs decoded: d_pack_off[0..nrun] = exclusive scan of d_run_len and run r's bytes
 * moved from d_out + out_off to d_packed + d_pack_off[r] (d_packed_bytes: its size; must not overlap d_out). */
int gpumt_lz4_pack_runs(gpumt_ctx *h, const void *d_out, size_t out_bytes, const gpumt_lz4_run *d_runs,
			const uint32_t *d_run_len, size_t nrun, void *d_packed, size_t packed_bytes,
			uint64_t *d_pack_off, int stream);

/*
 * XXH32 (seed 0) with carried state: job j continues a hash over d_base + off, len bytes.  GPUMT_XXH_RESET starts a new
 * hash, otherwise the state in slot GPUMT_XXH_IN of d_states (2 x GPUMT_XXH32_STATE_WORDS words of device memory: four
 * accumulators, up to 15 pending bytes, the total length) is continued; GPUMT_XXH_FINAL writes the digest to d_digest[j]
 * and, with GPUMT_XXH_VERIFY, GPUMT_ST_OK / GPUMT_ST_BAD_CHECKSUM against `expect` to d_verdict[j]; without it the
 * state goes to slot GPUMT_XXH_OUT.  One wave per job, the jobs of a call side by side: a call holds at most one job that
 * reads a state and one that leaves one, and they name different slots.  A job outside base_bytes: GPUMT_ST_BAD_RECORD.
 */
#define GPUMT_XXH32_STATE_WORDS 12
#define GPUMT_XXH_RESET 1u
#define GPUMT_XXH_FINAL 2u
#define GPUMT_XXH_VERIFY 4u
#define GPUMT_XXH_IN(slot) ((uint32_t)((slot) & 1) << 8)
#define GPUMT_XXH_OUT(slot) ((uint32_t)((slot) & 1) << 9)
typedef struct {
	uint64_t off;
	uint32_t len;
	uint32_t flags;
	uint32_t expect;
	uint32_t reserved;
} gpumt_xxh32_job;
int gpumt_xxh32_carry(gpumt_ctx *h, const void *d_base, size_t base_bytes, const gpumt_xxh32_job *d_jobs, size_t njobs,
		      uint32_t *d_states, uint32_t *d_digest, uint32_t *d_verdict, int stream);

/* ---- zstd-mt records (12-byte skippable header + one zstd frame, lib/zstd-mt_compress.c:296-302) ----
 *
 * gpumt_zstd_probe_sizes: d_out_len[i] = Frame_Content_Size of record i, d_out_off = exclusive
 * scan, d_status[i] = GPUMT_ST_OK or why the record cannot be decoded on the device (bad record /
 * frame header, or GPUMT_ST_UNSUPPORTED for frames without a content size -- zstd-mt always writes
 * one, it compresses each chunk with one-shot ZSTD_compress, :285).
 *
 * gpumt_zstd_decompress_batch: decode the records whose d_status is GPUMT_ST_OK (replaces
 * ZSTD_decompressStream at lib/zstd-mt_decompress.c:464): raw / RLE / compressed blocks, Huffman
 * literals, FSE sequence tables of every mode, repeat offsets, XXH64 content checksum (verified, a
 * mismatch reports GPUMT_ST_BAD_CHECKSUM); no dictionaries.  Same d_stream slack rule as above.
 * d_out_len[i] is the exact content size for frames that state one (what the probe returns); for a
 * frame without a content size (streaming writers, plain .zst files) the caller passes a capacity
 * there and the decoder replaces it by the decoded size.
 * out_bytes is the size of the output the batch produces (every record's [d_out_off[i], d_out_off[i] + d_out_len[i]) lies
 * inside it).
 * Internal scratch: GPUMT_ZSTD_DEC_SCRATCH (320 KiB) per record of a launch slice (at most 16384
 * records, 5 GiB) + 8 B per record; batches whose records average more than 128 KiB of content (frames of several blocks)
 * take out_bytes + 16 more for the sequence pre-pass (zmt_zstd_seq_kernel: the FSE sequence streams of a frame's blocks
 * decoded side by side ahead of the frame decoder; GPUMT_ZSTD_SEQ=1 or gpumt_set_variant(h, "zstd_seq", 1) turn it off).
 */
/* Bytes one zstd record slot occupies: room for the record + frame header and one padded area per
 * 128 KiB block (the blocks are compressed independently and then moved together), rounded to 256. */
size_t gpumt_zstd_slot_stride(size_t chunk);

/*
 * Compress n bytes at d_in (the allocation must extend 64 readable bytes past n) as independent
 * chunks of `chunk` bytes (last one shorter; n == 0 gives one empty chunk): record i (12-byte
 * skippable header + one zstd frame that decodes to chunk i; replaces ZSTD_compress at
 * lib/zstd-mt_compress.c:285 + header emit :296-302) is written at d_slots + i*slot_stride and its
 * length to d_rec_len[i].  gpumt_lz4_compact then packs the records into the MT stream.
 * The frames are valid RFC 8878 (single segment, content size, no checksum, blocks of at most
 * 128 KiB); their bytes are not those of libzstd -- the bar for zstd is decompress-identical.
 */
int gpumt_zstd_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk,
			      void *d_slots, size_t slot_stride, uint32_t *d_rec_len, int stream);
/* The same at `level` 1..22 (what the reference hands to ZSTD_compress, lib/zstd-mt_compress.c:285): the device encoder
 * has three tiers -- levels 1-2, 3-9, 10-22 (gpumt_zstd_level_tier = 0, 1, 2) -- that trade speed for ratio through
 * the size of the hash table and the number of bytes hashed; gpumt_zstd_compress_batch is level 1. */
int gpumt_zstd_level_tier(int level);
int gpumt_zstd_compress_batch_level(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				    size_t slot_stride, uint32_t *d_rec_len, int level, int stream);
/*
 * The same with the whole chunk as the match window (opt-in; what GPUMT_ZSTD_WIN=1 makes ZSTDCB_compressCCtx call at
 * levels 10-22).  Arguments, slot layout and records are those of gpumt_zstd_compress_batch_level, and levels below 10
 * are passed straight to it.  From level 10 on a first launch writes a chain plane -- per input byte the nearest earlier
 * position of the same chunk whose next 6 bytes hash alike -- and the block encoder walks it for up to
 * gpumt_zstd_win_depth(level) candidates per position (8 for levels 10-12, 16 for 13-15, 32 for 16-18, 64 for 19-22, 0
 * below 10; levels of one group give the same bytes) and keeps the best by 4 * length - log2(offset + 1), ties to the
 * nearer.  A match takes its source from any earlier byte of its chunk at a distance of at most 2^27, never from
 * another chunk, and ends with its 128 KiB block; the frames stay single-segment with a content size, so every offset
 * is legal.  The bytes depend on the input, the chunk and the level group alone: not on the grid nor on the other
 * records of the batch.
 * Internal scratch: GPUMT_ZSTD_WIN_SCRATCH(n) -- 4 bytes per input byte for the plane -- plus 512 KiB of head table per
 * resident wave of the first launch and the per-wave areas of gpumt_zstd_compress_batch_level.  A batch above 1 GiB is
 * processed in slices of whole records of at most 1 GiB of input each, so the plane never exceeds 4 GiB.  If the device
 * refuses the scratch the call encodes with gpumt_zstd_compress_batch_level, remembers the refused size (it is not
 * asked for again) and, like every call from level 10 on, says so in its GPUMT_TRACE=1 line: records, depth (0 = the
 * table encoder ran), plane bytes, fallback.  Chunks above 128 MiB, whose frames carry a 128 KiB Window_Descriptor,
 * take that path as well.
 * gpumt_set_variant(h, "zstd_win_depth", d) overrides the depth for A/B runs: 1..256, 0 = by level, anything else is
 * rejected (-1); "zstd_win_cap_mb" (0 = none) refuses scratch requests above that many MiB: the tests' way to the
 * fallback.
 */
#define GPUMT_ZSTD_WIN_SCRATCH(n) ((size_t)4 * (n) + 256)
int gpumt_zstd_win_depth(int level);
int gpumt_zstd_compress_batch_win(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				  size_t slot_stride, uint32_t *d_rec_len, int level, int stream);

/*
 * The chain plane of both window encoders on its own, and its segment-parallel build (opt-in).
 * gpumt_win_chain_plane writes the n words of the plane of d_in cut into chunks -- word p = the nearest earlier position of
 * p's chunk (chunk-relative) whose next 6 bytes hash alike, or 0xFFFFFFFF -- to d_plane; n <= 1 GiB, chunk <= 2^27, and d_in
 * has the encoders' readable slack behind it.  seg_log 0: one wave builds a chunk, 64 positions per step in order, as both _win
 * calls do by default.  seg_log 12..24: a chunk is cut into segments of 1 << seg_log positions, persistent waves chain each
 * segment over a head table of its own, a second launch carries the head tables forward through the chunk's segments and a
 * third gives every position without a predecessor in its segment the one the earlier segments hold: the same plane, word
 * for word, whatever the input (where no chunk has more than one segment the first kernel runs).  Anything else is
 * GPUMT_E_ARG.  The head tables take gpumt_win_chain_par_scratch(n, chunk, seg_log) bytes of internal scratch -- per segment
 * 4 << min(17, max(12, log2(min(chunk, n)) - 3)) bytes; 0 where the segment build does not run -- and this call never builds
 * the plane another way than asked: head tables the device or "win_chain_cap_mb" refuses are GPUMT_E_NOMEM.
 * gpumt_set_variant(h, "win_chain_par", k) makes gpumt_zstd_compress_batch_win and gpumt_brotli_compress_batch_win build
 * their plane in segments: 0 = off (the default), 1 = on at seg_log 20 (profiles/win_chain_par.txt), 12..24 = on at that seg_log, anything else is
 * rejected (-1); GPUMT_WIN_CHAIN_PAR in the environment holds the same values when the context is opened (unset, empty and
 * any other text = off).  Both calls then ask for their scratch with the head tables of the largest slice behind it first;
 * refused -- by the device, or above "win_chain_cap_mb" MiB (0 = none), the tests' way there -- they build the plane with one
 * wave per chunk, remember the refused size (not asked for again; a new cap asks again) and go on as without the variant.
 * The records are byte for byte those without the variant in every case.  With GPUMT_TRACE=1 a second line follows
 * theirs: `[gpumt win chain] segments N seg_log L heads B serial S` (the segments of the largest slice, the head-table
 * bytes asked for, S = 1 where one wave per chunk built the plane).
 */
size_t gpumt_win_chain_par_scratch(size_t n, size_t chunk, int seg_log);
int gpumt_win_chain_plane(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, uint32_t *d_plane, int seg_log,
			  int stream);

int gpumt_zstd_probe_sizes(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
			   const uint32_t *d_rec_len, size_t nrec, uint32_t *d_out_len,
			   uint64_t *d_out_off, uint32_t *d_status, int stream);
int gpumt_zstd_decompress_batch(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				const uint64_t *d_rec_off, const uint32_t *d_rec_len, size_t nrec,
				void *d_out, size_t out_bytes, const uint64_t *d_out_off,
				uint32_t *d_out_len, uint32_t *d_status, int stream);

/*
 * gpumt_zstd_decompress_batch with the records of several blocks decoded block-parallel (opt-in; what GPUMT_ZSTD_REC_PAR=1
 * makes ZSTDCB_decompressDCtx call).  Same arguments and slack rule, and for every record the same status, the same
 * d_out_len and the same output bytes: a frame without a content size passes a capacity and gets the decoded size back, a
 * record whose d_status is not GPUMT_ST_OK on entry is not visited, and nothing outside a record's
 * [d_out_off[i], d_out_off[i] + d_out_len[i]) is written.  d_rec_par (nrec words, may be NULL) receives per record the
 * number of its blocks whose result came from the block call (gpumt_zstd_decompress_blocks_par on the tables made here) and
 * was kept, 0 for every other record.  It says that the record went through that call, not which of that call's own routes
 * decoded it: the call leaves a run to its entropy stage or to its serial wave by its own rules (a run of one block, a
 * serial prefix, GPUMT_ZSTD_RUN_PAR=0 / GPUMT_ZSTD_RUN_PRE=0, a refused origin plane), with the same bytes.
 * A return value other than GPUMT_OK (the block call or the record decoders failed to launch) leaves the batch undefined:
 * d_status may not have been written, and d_out_len of records without a stated size may already hold decoded sizes.
 * The stages, stream-ordered, none of which waits on another wave:
 *   count   one lane per OK record checks the 12-byte header and the frame header (magic, descriptor, reserved bit,
 *           Window_Descriptor, Dictionary_ID, Frame_Content_Size) and hops from block header to block header until
 *           Last_Block, the end of the record or a block that would leave it.  A record is eligible when the walk ended on
 *           Last_Block, the frame has no Dictionary_ID field, a stated content size equals d_out_len[i], and it has
 *           zstd_rec_min_blocks .. 65536 blocks.  The stage decides no verdict.
 *   (host)  one copy of the counts to pinned memory and one hipStreamSynchronize of `stream`: the host cuts the batch into
 *           slices of consecutive records with at most 4096 eligible records, zstd_rec_slice_blocks blocks (a record of
 *           more is a slice of its own) and 0xFFFFFFF0 stream bytes.  A batch without an eligible record goes to the record
 *           decoders as it is.  A slice passes d_stream and d_out offset to its first eligible record (rounded down to 256), so
 *           the origin plane of the block call is 4 x the slice's output span.
 *   table   per slice a scan of the block counts, then one lane per eligible record writes its gpumt_zstd_block entries and
 *           one gpumt_zstd_run (hist 0, GPUMT_ZRUN_FIRST | GPUMT_ZRUN_LAST, carry 0, out_cap = d_out_len[i]).
 *   blocks  gpumt_zstd_decompress_blocks_par on the slice's tables, unchanged: it falls back by its own rules.
 *   finish  one lane per eligible record keeps it when the run's status is OK, its length is the stated content size, and
 *           behind the last block lie exactly the 4 checksum bytes the descriptor promises, or nothing.  A kept record
 *           gets d_out_len (no stated size), d_rec_par, its checksum words, and a skip value in a scratch copy of d_status.
 *   records the record decoders of gpumt_zstd_decompress_batch over the whole batch with that scratch copy: records that
 *           were not eligible or not kept are decoded and judged there, so the verdicts are the serial call's by
 *           construction.  A merge writes d_status (OK for kept records, else the decoders' word) and the XXH64 verify runs
 *           once over all records.
 * Internal scratch: areas of its own, which the block call and the record decoders do not replace -- 76 bytes per record
 * and, for the largest slice, 16 bytes per block and 40 per eligible record, plus 2 x GPUMT_ZSTD_CARRY_BYTES -- next to
 * theirs.  If the device refuses them the call is gpumt_zstd_decompress_batch (d_rec_par 0) and that size is not asked for
 * again.
 * gpumt_set_variant: "zstd_rec_par" 1 = default, 0 = the call is gpumt_zstd_decompress_batch with d_rec_par all 0;
 * "zstd_rec_min_blocks" 1..65536 (default 4: a placeholder, not a measurement; GPUMT_ZSTD_REC_MIN_BLOCKS);
 * "zstd_rec_slice_blocks" 2..65536 (default 4096; GPUMT_ZSTD_REC_SLICE_BLOCKS); "zstd_rec_cap_mb" (0 = none) refuses the
 * stage's own scratch above that many MiB, the tests' way to the fallback.  Values out of range are refused with -1 and
 * change nothing.  With GPUMT_TRACE=1 every call prints `[gpumt zstd rec] records N par P blocks B slices S fallback F`
 * (P eligible records with B blocks in S calls of the block stages; F = 1: this stage's own scratch was refused and the
 * record decoders took the whole batch -- the block call's own fallbacks are not counted here).
 */
int gpumt_zstd_decompress_batch_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				    const uint64_t *d_rec_off, const uint32_t *d_rec_len, size_t nrec,
				    void *d_out, size_t out_bytes, const uint64_t *d_out_off,
				    uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int stream);

/*
 * Block-level zstd decode: what the plain .zst path of ZSTDCB_decompressDCtx uses in place of one record per frame
 * (replaces the streaming ZSTD_decompressStream of st_decompress, lib/zstd-mt_decompress.c:552-687).  The caller walks the
 * frame and block headers and passes a table of blocks and a list of runs; a run is the consecutive blocks of one frame
 * that a call holds, and one wave decodes it, block after block, to d_out + out_off, at most out_cap bytes.
 *   a whole frame:          one run with GPUMT_ZRUN_FIRST | GPUMT_ZRUN_LAST; runs of different frames decode side by side
 *   a frame over several calls: its runs go one per call, in order.  What a later block may refer to -- the three repeat
 *                           offsets, the Huffman table (treeless literals), the LL / OF / ML tables (Repeat_Mode) -- is
 *                           left in slot `carry` (0 or 1) of d_carry (2 x GPUMT_ZSTD_CARRY_BYTES of device memory) unless
 *                           the run is LAST, and taken from there unless it is FIRST.  The caller places the last `hist`
 *                           bytes of the frame's earlier output (min(bytes so far, window)) directly in front of out_off:
 *                           a match may reach back that far and no further.  The runs of one call that name a carry slot
 *                           belong to different frames when they name different slots.
 * d_run_len[r] receives the bytes run r decoded, d_status[r] GPUMT_ST_OK, GPUMT_ST_BAD_BLOCK (malformed block, block
 * above block_max or above the room left, a match that reaches in front of the history, a treeless or Repeat_Mode block
 * whose table neither the run nor the carry holds, a run behind one that failed) or GPUMT_ST_BAD_RECORD (a table entry
 * that leaves stream_bytes / out_bytes, or whose src_len is not the length its block header states: the tables are device
 * memory, the kernel checks them).  Frame header, Frame_Content_Size and the content checksum are the caller's
 * (gpumt_xxh64_carry).  Same d_stream slack rule as gpumt_zstd_decompress_batch; stream_bytes below 4 GiB.
 * Internal scratch: GPUMT_ZSTD_RUN_SCRATCH bytes per run.
 */
#define GPUMT_ZRUN_FIRST 1u
#define GPUMT_ZRUN_LAST 2u
#define GPUMT_ZSTD_CARRY_BYTES 9280u
#define GPUMT_ZSTD_RUN_SCRATCH 131328u
typedef struct {
	uint64_t src_off;   /* the block's 3-byte header in d_stream */
	uint32_t src_len;   /* header + body (4 for an RLE block) */
	uint32_t block_max; /* min(the frame's window, 128 KiB) */
} gpumt_zstd_block;
typedef struct {
	uint64_t out_off;
	uint32_t out_cap;      /* hist + out_cap at most 0xFFFE0000: positions inside a run are 32 bits */
	uint32_t hist;         /* bytes of the frame's earlier output in front of out_off */
	uint32_t first, count; /* blocks [first, first + count) */
	uint32_t flags;        /* GPUMT_ZRUN_* */
	uint32_t carry;        /* slot of d_carry, 0 or 1 */
} gpumt_zstd_run;
int gpumt_zstd_decompress_blocks(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				 const gpumt_zstd_block *d_blocks, size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun,
				 void *d_out, size_t out_bytes, void *d_carry, uint32_t *d_run_len, uint32_t *d_status,
				 int stream);

/*
 * The same call with a block-parallel entropy stage in front of the runs: same arguments, contract, statuses, d_run_len and
 * carry as gpumt_zstd_decompress_blocks -- a call of either kind may follow a call of the other on the same carry.  Three
 * more launches on the same stream, none of which waits on another wave: one lane per block reads the block, literals and
 * sequences headers; one wave per run finds, for every block, the earlier block of the same run in this call that
 * describes the Huffman / LL / OF / ML table it uses (treeless literals, Repeat_Mode); one wave per Compressed_Block, all
 * blocks of all runs side by side, decodes the block's Huffman literals and its FSE sequence bitstream into scratch.  The
 * runs then decode one wave each as before, but a block the stage marked only builds its tables, copies its literals and
 * executes its sequences (repeat offsets, matches): what is still one chain per frame.
 * d_block_mark (nblk words, may be NULL) receives per block: bit 0 = its sequences were decoded ahead, bit 1 = its literals
 * were (or are raw / RLE literals, which need no decoding).  A block is marked only when its tables, bitstreams and
 * end-of-stream conditions were all clean; a Raw or RLE block, a block whose table was defined before this call (it is in
 * the carry), a block with more than block_max / 4 sequences, and anything malformed are 0 and decoded -- and judged --
 * exactly as gpumt_zstd_decompress_blocks does.
 * Internal scratch: GPUMT_ZSTD_RUN_SCRATCH per run + GPUMT_ZSTD_PRE_SCRATCH(131072) + 52 bytes per block of the table, whatever
 * the block's own size (the slots lie at one stride: 3 GiB for a table of 8192 blocks); when the device cannot provide it
 * the call decodes serially (marks 0) rather than fail, keeps the scratch it has, and does not ask for that size again.
 * GPUMT_ZSTD_RUN_PRE=0 in the environment or gpumt_set_variant(h, "zstd_run_pre", 0) turn the stage off: the call is then
 * gpumt_zstd_decompress_blocks with every mark 0 (1 turns it on again; other values are refused).
 */
/* what a block of the table needs: its literals (128 KiB + slack) and block_max / 4 sequences of 8 bytes */
#define GPUMT_ZSTD_PRE_SCRATCH(block_max) (131072u + 256u + 8u * ((block_max) / 4u))
int gpumt_zstd_decompress_blocks_pre(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				     const gpumt_zstd_block *d_blocks, size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun,
				     void *d_out, size_t out_bytes, void *d_carry, uint32_t *d_run_len, uint32_t *d_status,
				     uint32_t *d_block_mark, int stream);

/*
 * The same call with, behind the entropy stage, a block-parallel execute stage: same arguments, contract, statuses,
 * d_run_len, output bytes and carry as the two calls above -- a call of any of the three may follow a call of any other on
 * the same carry.  d_block_mark is that of gpumt_zstd_decompress_blocks_pre.  Per run, the blocks behind its last
 * Compressed_Block that is not fully marked (Raw, RLE and fully marked blocks) are its parallel suffix, the blocks in front
 * its serial prefix; a suffix of fewer than 2 blocks leaves the run to the serial wave.  The prefix decodes as before on a
 * scratch copy of the carry slot.  The suffix then takes stream-ordered launches, none of which waits on another wave:
 * measure (one wave per block: decoded size and the block's repeat-offset transfer function), scan (one wave per run:
 * positions, incoming repeat offsets, room), execute (one wave per block at its final position; a match source inside
 * another suffix block is not read, its run position + 1 goes into a plane of one u32 per output byte and travels with
 * copies inside the block), resolve (one workgroup per run, block after block, fills those bytes in) and carry (one wave
 * per run: the tables from the last block that describes each).  A run that any stage refuses -- and every failing run --
 * is decoded again by the serial wave from the caller's untouched carry slot, so its status, d_run_len, bytes and carry
 * are the serial call's.  What stays serial per frame: the block-order resolve and the prefix.
 * d_block_par (nblk words, may be NULL) receives 1 for every block whose bytes the parallel stage produced and kept.
 * Internal scratch: that of gpumt_zstd_decompress_blocks_pre + GPUMT_ZSTD_PAR_SCRATCH(out_bytes) + 48 bytes per block +
 * GPUMT_ZSTD_CARRY_BYTES + 84 bytes per run; when the device cannot provide it the call is
 * gpumt_zstd_decompress_blocks_pre (d_block_par 0) and that size is not asked for again.
 * The same holds for a table of more than 4096 runs (the pre call's own limit for its stage) and for a table without a run
 * of two or more blocks: d_block_par is all 0 then.
 * GPUMT_ZSTD_RUN_PAR=0 in the environment or gpumt_set_variant(h, "zstd_run_par", 0) turn the stage off the same way
 * (1 turns it on again; other values are refused).
 */
#define GPUMT_ZSTD_PAR_SCRATCH(out_bytes) (4 * (size_t)(out_bytes) + 16)
int gpumt_zstd_decompress_blocks_par(gpumt_ctx *h, const void *d_stream, size_t stream_bytes,
				     const gpumt_zstd_block *d_blocks, size_t nblk, const gpumt_zstd_run *d_runs, size_t nrun,
				     void *d_out, size_t out_bytes, void *d_carry, uint32_t *d_run_len, uint32_t *d_status,
				     uint32_t *d_block_mark, uint32_t *d_block_par, int stream);

/*
 * XXH64 (seed 0) with carried state, the content checksum of a zstd frame decoded over several calls: gpumt_xxh32_carry's
 * contract with the same job record and flags, a state of GPUMT_XXH64_STATE_WORDS words per slot (four 64-bit
 * accumulators, the total length, up to 31 pending bytes), and `expect` / d_digest are the low 32 bits of the hash --
 * what a zstd frame stores (RFC 8878 3.1.1).
 */
#define GPUMT_XXH64_STATE_WORDS 20
int gpumt_xxh64_carry(gpumt_ctx *h, const void *d_base, size_t base_bytes, const gpumt_xxh32_job *d_jobs, size_t njobs,
		      uint32_t *d_states, uint32_t *d_digest, uint32_t *d_verdict, int stream);

/* ---- brotli-mt records (16-byte header + one raw brotli stream, lib/brotli-mt_compress.c:285-304) ----
 *
 * gpumt_brotli_decompress_batch: decode nrec brotli streams (replaces BrotliDecoderDecompress at
 * lib/brotli-mt_decompress.c:344-346).  Stream i is d_stream + d_rec_off[i], d_rec_len[i] bytes (the
 * payload behind the 16-byte header, which the host parses while reading, :187-284); its output goes
 * to d_out + d_out_off[i] and may take d_out_cap[i] bytes (hint << 16, :236-239).  d_out_len[i]
 * receives the decoded size, d_status[i] GPUMT_ST_OK, GPUMT_ST_BAD_BLOCK (malformed / truncated
 * stream) or GPUMT_ST_SIZE_MISMATCH (output exceeds the capacity) -- the reference reports
 * frame_decompress for both.  Complete RFC 7932 decoder incl. the static dictionary.  Same
 * d_stream slack rule as above.  Internal scratch: GPUMT_BROTLI_SCRATCH bytes per resident wave.
 */
/* gpumt_brotli_compress_batch: chunk i = d_in[i*chunk, ...) -> one record (16-byte brotli-mt header with
 * the output hint, lib/brotli-mt_compress.c:285-304, + one raw brotli stream that decodes to the
 * chunk; replaces BrotliEncoderCompress at :269-272) at d_slots + i*slot_stride, its length to
 * d_rec_len[i]; slot_stride >= gpumt_zstd_slot_stride(chunk).  gpumt_lz4_compact packs the records.
 * The streams are valid RFC 7932 (window 2^18, one meta-block per 128 KiB with its own three prefix
 * codes, byte-aligned by empty metadata meta-blocks); their bytes are not libbrotli's -- the bar for
 * brotli is decompress-identical. */
int gpumt_brotli_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				size_t slot_stride, uint32_t *d_rec_len, int stream);
/* The same at quality `level` 0..11 (what the reference hands to BrotliEncoderCompress, lib/brotli-mt_compress.c:269-272):
 * three device tiers -- 0-3, 4-8, 9-11 (gpumt_brotli_level_tier = 0, 1, 2); gpumt_brotli_compress_batch is quality 1. */
int gpumt_brotli_level_tier(int level);
int gpumt_brotli_compress_batch_level(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				      size_t slot_stride, uint32_t *d_rec_len, int level, int stream);
/*
 * The same with the whole chunk as the match window (opt-in; what GPUMT_BROTLI_WIN=1 makes BROTLIMT_compressCCtx call at
 * qualities 9-11).  Arguments, slot layout and records are those of gpumt_brotli_compress_batch_level, and qualities below
 * 9 are passed straight to it.  From quality 9 on a first launch writes the chain plane of gpumt_zstd_compress_batch_win --
 * per input byte the nearest earlier position of the same chunk whose next 6 bytes hash alike; the same kernel -- and the
 * block encoder walks it for up to gpumt_brotli_win_depth(level) candidates per position (16 / 32 / 64 for qualities 9 /
 * 10 / 11, 0 below 9), measures each on 24 bytes and keeps the best by 4 * length - log2(distance + 1), ties to the nearer.
 * A match takes its source from any earlier byte of its chunk, never from another chunk, and ends with its 128 KiB
 * meta-block.  Every stream declares the smallest WBITS in 18..24 whose window, (1 << WBITS) - 16, holds the chunk's largest
 * distance (else 24), and no distance exceeds min(position in the chunk, that window), so none can be read as a reference
 * into the static dictionary; chunks above 16 MiB stay on this path and rely on the cap.  NPOSTFIX = NDIRECT = 0, no
 * context modelling, as before.  The bytes depend on the input, the chunk and the quality alone: not on the grid nor on the
 * other records of the batch.
 * Internal scratch: GPUMT_BROTLI_WIN_SCRATCH(n) -- 4 bytes per input byte for the plane -- plus 512 KiB of head table per
 * resident wave of the first launch and the per-wave areas of gpumt_brotli_compress_batch_level.  A batch above 1 GiB is
 * processed in slices of whole records of at most 1 GiB of input each.  If the device refuses the scratch the call encodes
 * with gpumt_brotli_compress_batch_level, remembers the refused size (it is not asked for again) and, like every call from
 * quality 9 on, says so in its GPUMT_TRACE=1 line: `[gpumt brotli win] records N depth D plane B fallback F` (depth 0 = the
 * table encoder ran).
 * gpumt_set_variant(h, "brotli_win_depth", d) overrides the depth for A/B runs: 1..256, 0 = by level, anything else is
 * rejected (-1); "brotli_win_cap_mb" (0 = none) refuses scratch requests above that many MiB: the tests' way to the
 * fallback.
 */
#define GPUMT_BROTLI_WIN_SCRATCH(n) ((size_t)4 * (n) + 256)
int gpumt_brotli_win_depth(int level);
int gpumt_brotli_compress_batch_win(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				    size_t slot_stride, uint32_t *d_rec_len, int level, int stream);

#define GPUMT_BROTLI_SCRATCH 825856u
/* zstd decode: scratch per record (literals of one 128 KiB unit + 24576 sequences decoded ahead) */
#define GPUMT_ZSTD_DEC_SCRATCH 327936u
int gpumt_brotli_decompress_batch(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
				  const uint32_t *d_rec_len, size_t nrec, void *d_out,
				  const uint64_t *d_out_off, const uint32_t *d_out_cap,
				  uint32_t *d_out_len, uint32_t *d_status, int stream);

/*
 * Records that say where they can be cut, and a decoder that spreads such a record over many waves (both opt-in; what
 * GPUMT_BROTLI_INDEX=1 and GPUMT_BROTLI_REC_PAR=1 make BROTLIMT_compressCCtx and BROTLIMT_decompressDCtx call).
 *
 * gpumt_brotli_compress_batch_index: gpumt_brotli_compress_batch_level -- same arguments, same block encoders -- with a span
 * index in every record of two blocks or more.  The index is one metadata meta-block (RFC 7932 section 9.2: every decoder
 * skips it) directly in front of the closing 0x03 byte.  It starts byte-aligned: ISLAST 0, MNIBBLES 11, reserved 0,
 * MSKIPBYTES nb, MSKIPLEN - 1 in nb bytes (the least nb that holds it), zero bits to the byte boundary -- nb + 1 bytes --
 * then, little endian, n entries { u32 comp_bytes, u32 out_bytes } and the trailer { u32 n, u32 0x58495242 "BRIX" }.  Span k
 * is stream bytes [sum comp_bytes[<k], + comp_bytes[k]) and decodes to out_bytes[k] bytes; span 0 starts at stream byte 0 with
 * the WBITS bits; one span is one 128 KiB block with its padding meta-block.  A reader finds the index from the record's
 * end: the last byte 0x03, the trailer in front of it, the body of 8 n + 8 bytes, the header.  The table encoders leave
 * every block self-contained (no match source and no reused distance from before the block), which is what makes the cut
 * valid; the window encoder (gpumt_brotli_compress_batch_win) does not, and writes no index.  A record of one block (and
 * the empty record) is byte for byte gpumt_brotli_compress_batch_level's.  The index costs 8 bytes per block and at most 12
 * more; csize in the 16-byte header includes it, the hint is unchanged, and gpumt_zstd_slot_stride(chunk) holds the record
 * at every chunk size (12 spare bytes per block, 15 per record); a record of more than 65536 blocks gets none.
 *
 * gpumt_brotli_decompress_batch_par: gpumt_brotli_decompress_batch -- same arguments, same d_status, d_out_len and output
 * bytes for every batch -- plus d_rec_par (nrec words, or NULL): 1 where the span stages produced the record, 0 where the
 * record decoders did.  The index is a hint and is never trusted.  Stages (csrc/hip/brotli_dec_rec.h, which also holds the
 * equivalence argument):
 *   plan     one lane per record: the index from the record's end, and its checks -- the magic, min_spans <= n <= 65536, no
 *            zero entry, sum comp_bytes + index block + 1 == d_rec_len, the bytes at sum comp_bytes are exactly the header
 *            above, sum out_bytes <= d_out_cap, WBITS.  A record that fails any of them is not eligible; no verdict here.
 *   table    the spans of all eligible records as units (stream range, output offset, WBITS), in slices of 2^20 units.
 *   execute  the dec4 scheme with a span as the unit: four spans per wave, one 16-lane group each, from the span's first
 *            byte to its last exactly, on a meta-block boundary.  A group refuses -- not a verdict -- what dec4 hands over
 *            (context modelling, block switching, large distance alphabets), an ISLAST bit inside the span, a meta-block
 *            across the span's end, a decoded length other than out_bytes, a copy whose source lies before the span's
 *            first output byte (every static dictionary reference is one) and, behind span 0, a distance code that
 *            reads a ring entry the span did not write.
 *   finish   a record is kept only if every span ended without refusal: d_out_len = sum out_bytes, GPUMT_ST_OK, d_rec_par 1.
 *   records  the pair of gpumt_brotli_decompress_batch over the whole batch, passing kept records by: every record not kept
 *            is decoded and judged there, so the verdicts are the serial call's by construction.
 * One host round trip (the plans, 32 bytes per record).  Own scratch: 36 bytes per record and 36 per span of the largest
 * slice; refused (or above "brotli_rec_cap_mb"), the whole batch goes to gpumt_brotli_decompress_batch and the size is
 * remembered.  gpumt_set_variant: "brotli_rec_par" (1 / 0 = the serial call alone), "brotli_rec_min_spans" (2..65536;
 * default 2 -- see profiles/brotli_rec_par.txt), "brotli_rec_cap_mb" (0 = none); anything else returns -1 and changes nothing.
 * GPUMT_TRACE=1 prints per call `[gpumt brotli rec] records N par P spans S kept K fallback F` (P eligible records, S their
 * spans, K records kept, F = 1 when scratch was refused).
 */
int gpumt_brotli_compress_batch_index(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				      size_t slot_stride, uint32_t *d_rec_len, int level, int stream);
int gpumt_brotli_decompress_batch_par(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
				      const uint32_t *d_rec_len, size_t nrec, void *d_out,
				      const uint64_t *d_out_off, const uint32_t *d_out_cap,
				      uint32_t *d_out_len, uint32_t *d_status, uint32_t *d_rec_par, int stream);

/* ---- snappy-mt records (16-byte header + one raw snappy stream, lib/snappy-mt_compress.c:280-300) ----
 *
 * gpumt_snappy_compress_batch: chunk i = d_in[i*chunk, ...) -> one record (header with the payload size,
 * "SP" and the reference's hint, + one raw snappy stream that decodes to the chunk; replaces
 * snappy_compress at lib/snappy-mt_compress.c:264-276) at d_slots + i*slot_stride, its length to
 * d_rec_len[i]; slot_stride >= gpumt_snappy_slot_stride(chunk) (16 + snappy_max_compressed_length).
 * gpumt_lz4_compact packs the records.  The streams are valid raw snappy (copies stay inside 64 KiB
 * blocks); their bytes are not those of the reference's snappy library, which is not part of its tree
 * -- the bar is decompress-identical.  d_in must extend 64 readable bytes past n.
 *
 * gpumt_snappy_decompress_batch: decode nrec raw snappy streams (replaces snappy_uncompress at
 * lib/snappy-mt_decompress.c:350).  Stream i is d_stream + d_rec_off[i], d_rec_len[i] bytes (the
 * payload behind the 16-byte header); its output goes to d_out + d_out_off[i] and may take
 * d_out_cap[i] bytes -- the caller reads the stream's varint preamble for it, as the reference does
 * (snappy_uncompressed_length, :262-267).  d_out_len[i] receives the decoded size, d_status[i]
 * GPUMT_ST_OK, GPUMT_ST_BAD_BLOCK (malformed / truncated stream, or not the size its preamble states)
 * or GPUMT_ST_SIZE_MISMATCH (the preamble exceeds the capacity).  Same d_stream slack rule as above. */
size_t gpumt_snappy_slot_stride(size_t chunk);
int gpumt_snappy_compress_batch(gpumt_ctx *h, const void *d_in, size_t n, size_t chunk, void *d_slots,
				size_t slot_stride, uint32_t *d_rec_len, int stream);
int gpumt_snappy_decompress_batch(gpumt_ctx *h, const void *d_stream, const uint64_t *d_rec_off,
				  const uint32_t *d_rec_len, size_t nrec, void *d_out,
				  const uint64_t *d_out_off, const uint32_t *d_out_cap,
				  uint32_t *d_out_len, uint32_t *d_status, int stream);

/* XXH32 (seed 0) of n items: item i = d_base + d_off[i], d_len[i] bytes -> d_hash[i]. */
int gpumt_xxh32_batch(gpumt_ctx *h, const void *d_base, const uint64_t *d_off,
		      const uint32_t *d_len, size_t n, uint32_t *d_hash, int stream);

/* Developer aid: read-and-clear the 16 phase-cycle counters filled by the profiling decoder
 * (gpumt_set_variant("lz4_dec", 2)). */
int gpumt_debug_counters(gpumt_ctx *h, unsigned long long *dst, int n);

/* Kernel-variant selector for A/B measurements (0 = default; "zstd_run_pre", "zstd_run_par", "lz4_run_par" and "lz4_block_seg":
 * 1 = default, 0 = off, anything else is refused with -1 and changes nothing; "lz4_seg_bytes": see
 * gpumt_lz4_decompress_blocks_seg). Returns previous value. */
int gpumt_set_variant(gpumt_ctx *h, const char *what, int variant);

#ifdef __cplusplus
}
#endif
#endif
