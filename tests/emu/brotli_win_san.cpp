/* TEST HARNESS ONLY: a stand-alone program over the emulator build of gpumt_brotli_compress_batch_win, meant to be compiled
 * with -fsanitize=address,undefined together with the kernels and the fiber runtime (tools/brotli_win_san.sh).  It reads the
 * cases tests/brotli_win.py dumps (the shape list at qualities 9 and 11, the far repeat, small chunks), encodes each with the
 * window encoder from heap buffers of exactly the contract's sizes -- the input with its 64 bytes of slack, one slot per
 * record -- at two grids, compares the records, and decodes them with the emulated decoder kernels. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
extern const unsigned char zmt_brotli_static[], zmt_brotli_static_end[];
size_t emu_zstd_slot_stride(size_t chunk);
uint32_t emu_brotli_compress_batch_win(const uint8_t *in, uint64_t n, uint32_t chunk, uint8_t *slots, uint64_t stride,
				       uint32_t *rec_len, uint32_t grid, int level, uint32_t depth, uint64_t cap);
void emu_brotli_decompress_batch(const uint8_t *stream, const uint64_t *rec_off, const uint32_t *rec_len, uint32_t nrec,
				 uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, uint32_t *status,
				 const uint8_t *blob, uint32_t grid);
}

int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f)
		return 2;
	uint32_t ncase = 0, bad = 0;
	uint64_t in_bytes = 0, out_bytes = 0;
	if (fread(&ncase, 4, 1, f) != 1)
		return 2;
	for (uint32_t c = 0; c < ncase; c++) {
		uint32_t h[3]; /* bytes, chunk, quality */
		if (fread(h, 4, 3, f) != 3)
			return 2;
		const uint32_t n = h[0], chunk = h[1], nrec = n ? (n + chunk - 1) / chunk : 1;
		std::vector<uint8_t> in((size_t)n + 64, 0xEE);
		if (n && fread(in.data(), 1, n, f) != n)
			return 2;
		const size_t stride = emu_zstd_slot_stride(chunk);
		std::vector<uint8_t> slots[2];
		std::vector<uint32_t> rl[2];
		bool same = true;
		for (int k = 0; k < 2; k++) {
			slots[k].assign(nrec * stride, 0xEE);
			rl[k].assign(nrec, 0xA5A5A5A5u);
			same = same && emu_brotli_compress_batch_win(in.data(), n, chunk, slots[k].data(), stride, rl[k].data(), k ? 1 : 3,
								     (int)h[2], 0, 0) != 0;
		}
		same = same && rl[0] == rl[1];
		/* the payloads (behind the 16-byte record headers) packed into a stream with 300 readable bytes behind it, as the
		 * decoder's contract has it; capacities from the headers' hints */
		std::vector<uint8_t> stream;
		std::vector<uint64_t> ro(nrec), oo(nrec + 1, 0);
		std::vector<uint32_t> pl(nrec), cap(nrec);
		for (uint32_t r = 0; same && r < nrec; r++) {
			const uint8_t *rec = slots[0].data() + r * stride;
			same = rl[0][r] <= stride && rl[0][r] > 16 && !memcmp(rec, slots[1].data() + r * stride, rl[0][r]);
			if (!same)
				break;
			ro[r] = stream.size();
			pl[r] = rl[0][r] - 16;
			cap[r] = (uint32_t)(rec[14] | rec[15] << 8) << 16;
			oo[r + 1] = oo[r] + cap[r];
			stream.insert(stream.end(), rec + 16, rec + rl[0][r]);
		}
		if (same) {
			const size_t sb = stream.size();
			stream.resize(sb + 300, 0xEE);
			std::vector<uint32_t> ol(nrec, 0), st(nrec, 99);
			std::vector<uint8_t> out((size_t)oo[nrec] + 64, 0xCC);
			emu_brotli_decompress_batch(stream.data(), ro.data(), pl.data(), nrec, out.data(), oo.data(), cap.data(), ol.data(),
						    st.data(), zmt_brotli_static, 2);
			uint64_t got = 0;
			for (uint32_t r = 0; r < nrec; r++) {
				same = same && st[r] == 0 && ol[r] <= cap[r] &&
				       !memcmp(out.data() + oo[r], in.data() + (size_t)r * chunk, ol[r]);
				got += ol[r];
			}
			same = same && got == n;
			in_bytes += n;
			out_bytes += sb;
		}
		if (!same) {
			fprintf(stderr, "case %u (%u bytes, chunk %u, quality %u) fails\n", c, n, chunk, h[2]);
			bad++;
		}
	}
	fclose(f);
	printf("%u cases, %u fail, %llu bytes in, %llu bytes of streams\n", ncase, bad, (unsigned long long)in_bytes,
	       (unsigned long long)out_bytes);
	return bad != 0;
}
