"""GPUMT_BROTLI_WIN through BROTLIMT_compressCCtx over the emulated device boundary: quality 11 with the variable set to 1,
unset and holding other text, and quality 5."""
import brotli_win_api as A
import emu_driver as E


def _decode(stream):
    recs, status = E.brotli_decompress(stream)
    assert (status == 0).all()
    return b"".join(recs)


def test_api_legs():
    A.check_legs("emu", _decode)
