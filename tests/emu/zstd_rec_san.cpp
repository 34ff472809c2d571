/* TEST HARNESS ONLY: a stand-alone program over the emulator build of gpumt_zstd_decompress_batch_par, meant to be compiled
 * with -fsanitize=address,undefined together with the kernels and the fiber runtime (tools/zstd_rec_san.sh).  It reads the
 * batches tests/zstd_rec.py dumps (the mixed batch whole and in slices, the frame-level edges, the damaged records), decodes
 * each with the record decoders and with the block-parallel record call into heap buffers of exactly the contract's sizes,
 * and compares status, d_out_len and bytes. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void emu_zstd_decompress_batch(const uint8_t *stream, uint64_t stream_bytes, const uint64_t *rec_off, const uint32_t *rec_len,
			       uint32_t nrec, uint8_t *out, const uint64_t *out_off, uint32_t *out_len, uint32_t *status);
void emu_zstd_decompress_batch_par(const uint8_t *stream, uint64_t stream_bytes, const uint64_t *rec_off, const uint32_t *rec_len,
				   uint32_t nrec, uint8_t *out, uint64_t out_bytes, const uint64_t *out_off, uint32_t *out_len,
				   uint32_t *status, uint32_t *rec_par, uint32_t min_blocks, uint32_t slice_blocks, int par_on,
				   uint32_t cap_mb, uint32_t *stats);
}

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	uint32_t ncase = 0, bad = 0, nrecs = 0, npar = 0, nfail = 0, nslice = 0;
	if (fread(&ncase, 4, 1, f) != 1)
		return 2;
	for (uint32_t c = 0; c < ncase; c++) {
		uint32_t h[5]; /* stream bytes, records, out bytes, min_blocks, slice_blocks */
		if (fread(h, 4, 5, f) != 5)
			return 2;
		const uint32_t n = h[1];
		std::vector<uint8_t> stream((size_t)h[0] + 256, 0xEE); /* the contract's slack behind the stream */
		std::vector<uint64_t> ro(n), oo(n);
		std::vector<uint32_t> rl(n), cap(n), st_in(n);
		if (fread(stream.data(), 1, h[0], f) != h[0] || fread(ro.data(), 8, n, f) != n || fread(rl.data(), 4, n, f) != n ||
		    fread(oo.data(), 8, n, f) != n || fread(cap.data(), 4, n, f) != n || fread(st_in.data(), 4, n, f) != n)
			return 2;
		std::vector<uint8_t> out[2];
		std::vector<uint32_t> ol[2] = {cap, cap}, st[2] = {st_in, st_in}, par(n, 0xA5A5A5A5u);
		uint32_t stats[5] = {0};
		for (int k = 0; k < 2; k++)
			out[k].assign(h[2], 0xCC); /* exactly out_bytes: a byte behind it is the sanitizer's to find */
		emu_zstd_decompress_batch(stream.data(), h[0], ro.data(), rl.data(), n, out[0].data(), oo.data(), ol[0].data(),
					  st[0].data());
		emu_zstd_decompress_batch_par(stream.data(), h[0], ro.data(), rl.data(), n, out[1].data(), h[2], oo.data(), ol[1].data(),
					      st[1].data(), par.data(), h[3], h[4], 1, 0, stats);
		bool same = ol[0] == ol[1] && st[0] == st[1];
		std::vector<uint8_t> inside(h[2], 0);
		for (uint32_t r = 0; r < n; r++) {
			for (uint32_t i = 0; i < cap[r]; i++)
				inside[oo[r] + i] = 1;
			if (st_in[r] != 0)
				same = same && par[r] == 0;
			else if (st[0][r] == 0)
				same = same && !memcmp(out[0].data() + oo[r], out[1].data() + oo[r], ol[0][r]);
			nfail += st[0][r] != 0;
			npar += par[r] != 0;
		}
		for (size_t i = 0; i < inside.size(); i++)
			same = same && (inside[i] || out[1][i] == 0xCC);
		nrecs += n;
		nslice += stats[3];
		if (!same) {
			fprintf(stderr, "case %u differs\n", c);
			bad++;
		}
	}
	fclose(f);
	printf("%u batches of %u records, %u differ, %u failing records among them, %u records decoded block-parallel in %u slices\n",
	       ncase, nrecs, bad, nfail, npar, nslice);
	return bad != 0;
}
