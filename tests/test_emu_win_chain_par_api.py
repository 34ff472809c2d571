"""GPUMT_WIN_CHAIN_PAR through ZSTDCB_compressCCtx (level 19) and BROTLIMT_compressCCtx (quality 11) over the emulated
device boundary: set to 12, unset and holding other text."""
import pytest

import emu_driver as E
import win_chain_api as A


def _decode_zstd(stream):
    out, status = E.zstd_decompress(stream)
    assert (status == 0).all()
    return out


def _decode_brotli(stream):
    recs, status = E.brotli_decompress(stream)
    assert (status == 0).all()
    return b"".join(recs)


@pytest.mark.parametrize("codec", sorted(A.CODECS))
def test_api_legs(codec):
    A.check_legs("emu", codec, _decode_zstd if codec == "zstd" else _decode_brotli)
