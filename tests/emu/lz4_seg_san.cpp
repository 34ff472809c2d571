/* TEST HARNESS ONLY: a stand-alone program over the emulator build of gpumt_lz4_decompress_blocks_seg, meant to be compiled
 * with -fsanitize=address,undefined together with lz4_dec.hip and the fiber runtime (tools/lz4_seg_san.sh).  It reads the
 * cases tests/lz4_seg.py dumps (hand-built blocks on segment cuts, failures in a later segment, linked runs), decodes each
 * with the serial and with the segment-parallel call into heap buffers of exactly the contract's sizes, and compares status,
 * run length, block lengths and bytes. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void emu_lz4_decompress_blocks(const uint8_t *stream, uint64_t stream_bytes, const void *blocks, uint32_t nblk, const void *runs,
			       uint32_t nrun, uint8_t *out, uint64_t out_bytes, uint32_t *blk_len, uint32_t *run_len, uint32_t *status);
void emu_lz4_decompress_blocks_seg(const uint8_t *stream, uint64_t stream_bytes, const void *blocks, uint32_t nblk,
				   const void *runs, uint32_t nrun, uint8_t *out, uint64_t out_bytes, uint32_t *blk_len,
				   uint32_t *run_len, uint32_t *status, uint32_t *block_seg, int seg_on, uint32_t seg_bytes);
}

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	uint32_t ncase = 0, bad = 0, nseg = 0, nfail = 0;
	if (fread(&ncase, 4, 1, f) != 1)
		return 2;
	for (uint32_t c = 0; c < ncase; c++) {
		uint32_t h[6]; /* stream bytes, blocks, runs, out bytes, front bytes, seg_bytes */
		if (fread(h, 4, 6, f) != 6)
			return 2;
		std::vector<uint8_t> stream(h[0]), blocks(h[1] * 24u), runs(h[2] * 32u), front(h[4]);
		if ((h[0] && fread(stream.data(), 1, h[0], f) != h[0]) || fread(blocks.data(), 24, h[1], f) != h[1] ||
		    fread(runs.data(), 32, h[2], f) != h[2] || (h[4] && fread(front.data(), 1, h[4], f) != h[4]))
			return 2;
		std::vector<uint8_t> out[2];
		std::vector<uint32_t> bl[2], rl[2], st[2], seg(h[1]);
		for (int k = 0; k < 2; k++) {
			out[k].assign((size_t)h[3], 0xCC); /* exactly out_bytes: one byte more is the sanitizer's */
			if (h[4])
				memcpy(out[k].data(), front.data(), h[4]);
			bl[k].assign(h[1], 0x5E5E5E5Eu);
			rl[k].assign(h[2], 0xA5A5A5A5u);
			st[k].assign(h[2], 99);
		}
		emu_lz4_decompress_blocks(stream.data(), h[0], blocks.data(), h[1], runs.data(), h[2], out[0].data(), h[3],
					  bl[0].data(), rl[0].data(), st[0].data());
		emu_lz4_decompress_blocks_seg(stream.data(), h[0], blocks.data(), h[1], runs.data(), h[2], out[1].data(), h[3],
					      bl[1].data(), rl[1].data(), st[1].data(), seg.data(), 1, h[5]);
		bool same = rl[0] == rl[1] && st[0] == st[1] && bl[0] == bl[1];
		for (uint32_t r = 0; same && r < h[2]; r++) {
			uint64_t off;
			memcpy(&off, runs.data() + 32u * r + 8, 8);
			same = off + rl[0][r] <= h[3] && !memcmp(out[0].data() + off, out[1].data() + off, rl[0][r]);
			nfail += st[0][r] != 0;
		}
		for (uint32_t b = 0; b < h[1]; b++)
			nseg += seg[b];
		if (!same) {
			fprintf(stderr, "case %u differs\n", c);
			bad++;
		}
	}
	fclose(f);
	printf("%u cases, %u differ, %u failing runs among them, %u segments decoded side by side\n", ncase, bad, nfail, nseg);
	return bad != 0;
}
