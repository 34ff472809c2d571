"""tests/test_emu_win_chain_par_api.py's legs through the library on the device: GPUMT_WIN_CHAIN_PAR=12, unset and other text."""
import pytest

import emu_driver as E
import win_chain_api as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("codec", sorted(A.CODECS))
def test_api_legs(codec):
    import zstdmt_amd as z
    eng = z.Engine(0)
    try:
        def decode(stream):
            if codec == "zstd":
                ro, rl = E.walk_records(stream)
                out, status = eng.decompress_bytes(stream, ro, rl, codec="zstd")
                assert (status == 0).all()
                return out
            ro, rl, cap = E.walk_brotli_records(stream)
            recs, status = eng.brotli_decompress_bytes(stream, ro, rl, cap)
            assert (status == 0).all()
            return b"".join(recs)
        A.check_legs("gpu", codec, decode)
    finally:
        eng.close()
