"""GPUMT_LZ4_REC_PAR through LZ4MT_decompressDCtx over the emulated device boundary: the variable set to 1, unset and
holding other text, the seg route, and every record a batch of its own."""
import lz4_rec_api as A


def test_api_legs():
    A.check_legs("emu")
