/* TEST HARNESS ONLY: a stand-alone program over the emulator build of gpumt_brotli_decompress_batch_par, meant to be compiled
 * with -fsanitize=address,undefined together with the kernels and the fiber runtime (tools/brotli_rec_san.sh).  It reads the
 * batches tests/brotli_rec.py dumps (own indexed records, foreign flushed streams with an index, every tampered record between
 * intact ones), decodes each with the record decoders and with the span call -- whole and in slices of six spans -- into heap
 * buffers of exactly the contract's sizes, and compares status, d_out_len and the bytes of the records that decoded. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void emu_brotli_decompress_batch(const uint8_t *stream, const uint64_t *rec_off, const uint32_t *rec_len, uint32_t nrec, uint8_t *out,
				 const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, uint32_t *status,
				 const uint8_t *blob, uint32_t grid);
void emu_brotli_decompress_batch_par(const uint8_t *stream, const uint64_t *rec_off, const uint32_t *rec_len, uint32_t nrec,
				     uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, uint32_t *status,
				     uint32_t *rec_par, const uint8_t *blob, uint32_t grid, uint32_t min_spans, uint64_t cap,
				     uint32_t slice_spans, uint64_t info[4]);
}

int main(int argc, char **argv)
{
	if (argc != 3)
		return 2;
	FILE *f = fopen(argv[1], "rb"), *fb = fopen(argv[2], "rb"); /* the cases; the RFC 7932 constant data */
	if (!f || !fb)
		return 2;
	std::vector<uint8_t> blob(1 << 20);
	blob.resize(fread(blob.data(), 1, blob.size(), fb));
	uint32_t ncase = 0, bad = 0, nrecs = 0, nkept = 0, nfail = 0;
	if (fread(&ncase, 4, 1, f) != 1)
		return 2;
	for (uint32_t c = 0; c < ncase; c++) {
		uint32_t n = 0;
		if (fread(&n, 4, 1, f) != 1)
			return 2;
		std::vector<uint8_t> stream;
		std::vector<uint64_t> ro(n), oo(n);
		std::vector<uint32_t> rl(n), cap(n);
		uint64_t out_bytes = 0;
		for (uint32_t r = 0; r < n; r++) {
			uint32_t h[2]; /* payload bytes, capacity */
			if (fread(h, 4, 2, f) != 2)
				return 2;
			ro[r] = stream.size();
			rl[r] = h[0];
			stream.resize(stream.size() + h[0]);
			if (fread(stream.data() + ro[r], 1, h[0], f) != h[0])
				return 2;
			oo[r] = out_bytes;
			cap[r] = h[1];
			out_bytes += h[1];
		}
		const size_t slen = stream.size();
		stream.resize(slen + 256, 0xEE); /* the contract's slack behind the stream */
		for (uint32_t slice = 0; slice < 2; slice++) {
			std::vector<uint8_t> out[2];
			std::vector<uint32_t> ol[2], st[2], par(n, 0xA5A5A5A5u);
			uint64_t info[4];
			for (int k = 0; k < 2; k++) {
				out[k].assign(out_bytes, 0xCC); /* exactly the areas: a byte behind them is the sanitizer's to find */
				ol[k].assign(n, 0xFFFFFFFFu);
				st[k].assign(n, 99u);
			}
			emu_brotli_decompress_batch(stream.data(), ro.data(), rl.data(), n, out[0].data(), oo.data(), cap.data(), ol[0].data(),
						    st[0].data(), blob.data(), 2);
			emu_brotli_decompress_batch_par(stream.data(), ro.data(), rl.data(), n, out[1].data(), oo.data(), cap.data(),
							ol[1].data(), st[1].data(), par.data(), blob.data(), 2, 2, 0, slice ? 6u : 1u << 20, info);
			bool same = st[0] == st[1];
			for (uint32_t r = 0; r < n; r++) {
				if (st[0][r] == 0)
					same = same && ol[0][r] == ol[1][r] && !memcmp(out[0].data() + oo[r], out[1].data() + oo[r], ol[0][r]);
				else
					nfail += !slice;
				same = same && par[r] <= 1 && (!par[r] || st[1][r] == 0);
				nkept += !slice && par[r];
			}
			nrecs += slice ? 0 : n;
			if (!same) {
				fprintf(stderr, "case %u (slices %u): the span call differs from the record decoders\n", c, slice);
				bad++;
			}
		}
	}
	printf("%u batches, %u records, %u kept by the span stages, %u with a verdict other than OK: %s\n", ncase, nrecs, nkept, nfail,
	       bad ? "MISMATCH" : "identical");
	return bad ? 1 : 0;
}
