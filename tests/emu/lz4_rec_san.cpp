/* TEST HARNESS ONLY: a stand-alone program over the emulator build of gpumt_lz4_decompress_batch_par, meant to be compiled
 * with -fsanitize=address,undefined together with the kernels and the fiber runtime (tools/lz4_rec_san.sh).  It reads the
 * batches tests/lz4_rec.py dumps (the mixed batch whole, in slices and on the seg route, the frame-level edges, the slice
 * batch), decodes each with the record decoders and with the block-parallel record call into heap buffers of exactly the
 * contract's sizes, and compares status, d_out_len and the bytes of the records that decoded. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void emu_lz4_decompress_batch(int variant, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *rec_off,
			      const uint32_t *rec_len, uint32_t nrec, uint8_t *out, uint64_t out_bytes, const uint64_t *out_off,
			      uint32_t *out_len, uint32_t *status);
void emu_lz4_decompress_batch_par(int variant, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *rec_off,
				  const uint32_t *rec_len, uint32_t nrec, uint8_t *out, uint64_t out_bytes, const uint64_t *out_off,
				  uint32_t *out_len, uint32_t *status, uint32_t *rec_par, uint32_t min_blocks, uint32_t slice_blocks,
				  int par_on, int seg_on, uint32_t seg_bytes, uint32_t cap_mb, uint32_t *stats);
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
		uint32_t h[7]; /* stream bytes, records, out bytes, min_blocks, slice_blocks, seg, seg_bytes */
		if (fread(h, 4, 7, f) != 7)
			return 2;
		const uint32_t n = h[1];
		std::vector<uint8_t> stream((size_t)h[0] + 256, 0xEE); /* the contract's slack behind the stream */
		std::vector<uint64_t> ro(n), oo(n);
		std::vector<uint32_t> rl(n), cap(n);
		if (fread(stream.data(), 1, h[0], f) != h[0] || fread(ro.data(), 8, n, f) != n || fread(rl.data(), 4, n, f) != n ||
		    fread(oo.data(), 8, n, f) != n || fread(cap.data(), 4, n, f) != n)
			return 2;
		/* both pipelines of the record decoders: frames + parse4 + copy3, and the wave-per-record kernel alone */
		for (int variant = 0; variant < 2; variant++) {
			std::vector<uint8_t> out[2];
			std::vector<uint32_t> ol[2] = {cap, cap}, st[2], par(n, 0xA5A5A5A5u);
			uint32_t stats[5] = {0};
			for (int k = 0; k < 2; k++) {
				out[k].assign(h[2], 0xCC); /* exactly out_bytes: a byte behind it is the sanitizer's to find */
				st[k].assign(n, 99u);
			}
			emu_lz4_decompress_batch(variant, stream.data(), h[0], ro.data(), rl.data(), n, out[0].data(), h[2], oo.data(),
						 ol[0].data(), st[0].data());
			emu_lz4_decompress_batch_par(variant, stream.data(), h[0], ro.data(), rl.data(), n, out[1].data(), h[2], oo.data(),
						     ol[1].data(), st[1].data(), par.data(), h[3], h[4], 1, (int)h[5], h[6], 0, stats);
			bool same = ol[0] == ol[1] && st[0] == st[1];
			std::vector<uint8_t> inside(h[2], 0);
			for (uint32_t r = 0; r < n; r++) {
				for (uint32_t i = 0; i < cap[r]; i++)
					inside[oo[r] + i] = 1;
				if (st[0][r] == 0)
					same = same && !memcmp(out[0].data() + oo[r], out[1].data() + oo[r], ol[0][r]);
				nfail += st[0][r] != 0;
				npar += par[r] != 0;
			}
			for (size_t i = 0; i < inside.size(); i++)
				same = same && (inside[i] || out[1][i] == 0xCC);
			nrecs += n;
			nslice += stats[3];
			if (!same) {
				fprintf(stderr, "case %u variant %d differs\n", c, variant);
				bad++;
			}
		}
	}
	fclose(f);
	printf("%u batches (each with both record pipelines), %u records, %u differ, %u failing records among them, %u records "
	       "decoded block-parallel in %u slices\n", ncase, nrecs, bad, nfail, npar, nslice);
	return bad != 0;
}
