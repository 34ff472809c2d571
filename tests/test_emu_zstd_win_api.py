"""GPUMT_ZSTD_WIN through ZSTDCB_compressCCtx over the emulated device boundary: level 19 with the variable set to 1,
unset and holding other text, and level 5."""
import emu_driver as E
import zstd_win_api as A


def _decode(stream):
    out, status = E.zstd_decompress(stream)
    assert (status == 0).all()
    return out


def test_api_legs():
    A.check_legs("emu", _decode)
