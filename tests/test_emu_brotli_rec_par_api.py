"""GPUMT_BROTLI_INDEX / GPUMT_BROTLI_REC_PAR / GPUMT_BROTLI_REC_MIN_SPANS through BROTLIMT_* over the emulated device
boundary: a round trip at a 1 MiB chunk, the callback trace with and without the par decoder, the reference build on the
indexed stream, and the variables holding other text."""
import brotli_rec_api as A


def test_api_legs():
    A.check_legs("emu")
