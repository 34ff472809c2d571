/* TEST HARNESS ONLY: a stand-alone program over the emulator build of the segment-parallel chain build
 * (enc_win_chain_par.h), meant to be compiled with -fsanitize=address,undefined together with the kernels and the fiber
 * runtime (tools/win_chain_par_san.sh).  It reads the cases tests/win_chain.py dumps (its shape list), builds each plane at
 * seg_log 12 and two grids from heap buffers of exactly the contract's sizes -- the input with its 64 bytes of slack, one
 * word per input byte, the head tables emu_win_chain_par sizes itself -- and compares it with the serial kernel's. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void emu_zstd_win_chain(const uint8_t *in, uint64_t n, uint32_t chunk, uint32_t *plane, uint32_t grid);
void emu_win_chain_par(const uint8_t *in, uint64_t n, uint32_t chunk, uint32_t *plane, uint32_t seg_log, uint32_t grid);
uint64_t emu_win_chain_par_scratch(uint64_t n, uint32_t chunk, uint32_t seg_log);
}

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	uint32_t ncase = 0, bad = 0, par = 0;
	uint64_t words = 0;
	if (fread(&ncase, 4, 1, f) != 1)
		return 2;
	for (uint32_t c = 0; c < ncase; c++) {
		uint32_t h[2]; /* bytes, chunk */
		if (fread(h, 4, 2, f) != 2)
			return 2;
		const uint32_t n = h[0], chunk = h[1];
		std::vector<uint8_t> in((size_t)n + 64, 0xEE);
		if (n && fread(in.data(), 1, n, f) != n)
			return 2;
		std::vector<uint32_t> want(n, 0xA5A5A5A5u);
		emu_zstd_win_chain(in.data(), n, chunk, want.data(), 3);
		bool same = true;
		for (uint32_t grid = 1; grid <= 3; grid += 2) {
			std::vector<uint32_t> got(n, 0x5A5A5A5Au);
			emu_win_chain_par(in.data(), n, chunk, got.data(), 12, grid);
			same = same && got == want;
		}
		par += emu_win_chain_par_scratch(n, chunk, 12) != 0;
		words += n;
		if (!same) {
			fprintf(stderr, "case %u (%u bytes, chunk %u) fails\n", c, n, chunk);
			bad++;
		}
	}
	fclose(f);
	printf("%u cases (%u through the segment build), %u fail, %llu words compared at two grids\n", ncase, par, bad,
	       (unsigned long long)words);
	return bad != 0;
}
