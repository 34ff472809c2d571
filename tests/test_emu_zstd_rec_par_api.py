"""GPUMT_ZSTD_REC_PAR through ZSTDCB_decompressDCtx over the emulated device boundary: the variable set to 1, unset and
holding other text, one thread, and every record a batch of its own."""
import zstd_rec_api as A


def test_api_legs():
    A.check_legs("emu")
