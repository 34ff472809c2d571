/* TEST HARNESS ONLY: a stand-alone program over the emulator build of gpumt_zstd_decompress_blocks_par, meant to be compiled
 * with -fsanitize=address,undefined together with zstd_dec.hip and the fiber runtime (tools/zstd_par_san.sh).  It reads the
 * cases tests/zstd_par.py dumps (hand-built frames at every cut, damaged streams), decodes each with the serial and with the
 * block-parallel call into heap buffers of exactly the contract's sizes, and compares status, run length and bytes. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void emu_zstd_decompress_blocks(const uint8_t *stream, uint64_t stream_bytes, const void *blocks, uint32_t nblk, const void *runs,
				uint32_t nrun, uint8_t *out, uint64_t out_bytes, uint8_t *carry, uint32_t *run_len, uint32_t *status);
void emu_zstd_decompress_blocks_par(const uint8_t *stream, uint64_t stream_bytes, const void *blocks, uint32_t nblk,
				    const void *runs, uint32_t nrun, uint8_t *out, uint64_t out_bytes, uint8_t *carry,
				    uint32_t *run_len, uint32_t *status, uint32_t *block_mark, uint32_t *block_par, int par_on);
}

#define CARRY 9280u

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	uint32_t ncase = 0, bad = 0, npar = 0, nfail = 0;
	if (fread(&ncase, 4, 1, f) != 1)
		return 2;
	for (uint32_t c = 0; c < ncase; c++) {
		uint32_t h[6]; /* stream bytes, blocks, runs, out bytes, history bytes, carry given */
		if (fread(h, 4, 6, f) != 6)
			return 2;
		std::vector<uint8_t> stream(h[0] + 256, 0xEE), blocks(h[1] * 16u), runs(h[2] * 32u), hist(h[4]), cy(2 * CARRY, 0xA5);
		if ((h[0] && fread(stream.data(), 1, h[0], f) != h[0]) || fread(blocks.data(), 16, h[1], f) != h[1] ||
		    fread(runs.data(), 32, h[2], f) != h[2] || (h[4] && fread(hist.data(), 1, h[4], f) != h[4]) ||
		    (h[5] && fread(cy.data(), 1, 2 * CARRY, f) != 2 * CARRY))
			return 2;
		std::vector<uint8_t> out[2], carry[2] = {cy, cy};
		std::vector<uint32_t> rl[2], st[2], mark(h[1] + 1), par(h[1] + 1);
		for (int k = 0; k < 2; k++) {
			out[k].assign((size_t)h[3] + 64, 0xCC);
			if (h[4])
				memcpy(out[k].data(), hist.data(), h[4]);
			rl[k].assign(h[2], 0xA5A5A5A5u);
			st[k].assign(h[2], 99);
		}
		emu_zstd_decompress_blocks(stream.data(), h[0], blocks.data(), h[1], runs.data(), h[2], out[0].data(), h[3],
					   carry[0].data(), rl[0].data(), st[0].data());
		emu_zstd_decompress_blocks_par(stream.data(), h[0], blocks.data(), h[1], runs.data(), h[2], out[1].data(), h[3],
					       carry[1].data(), rl[1].data(), st[1].data(), mark.data(), par.data(), 1);
		bool same = rl[0] == rl[1] && st[0] == st[1];
		for (size_t i = h[3]; i < out[1].size(); i++)
			same = same && out[1][i] == 0xCC;
		for (uint32_t r = 0; same && r < h[2]; r++) {
			uint64_t off;
			uint32_t hs;
			memcpy(&off, runs.data() + 32u * r, 8);
			memcpy(&hs, runs.data() + 32u * r + 12, 4);
			(void)hs;
			same = off + rl[0][r] <= h[3] && !memcmp(out[0].data() + off, out[1].data() + off, rl[0][r]);
			nfail += st[0][r] != 0;
		}
		for (uint32_t b = 0; b < h[1]; b++)
			npar += par[b];
		if (!same) {
			fprintf(stderr, "case %u differs\n", c);
			bad++;
		}
	}
	fclose(f);
	printf("%u cases, %u differ, %u failing runs among them, %u blocks decoded block-parallel\n", ncase, bad, nfail, npar);
	return bad != 0;
}
