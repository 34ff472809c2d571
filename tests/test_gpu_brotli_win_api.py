"""tests/test_emu_brotli_win_api.py's legs through the library on the device: GPUMT_BROTLI_WIN=1, unset and other text."""
import pytest

import brotli_win_api as A
import emu_driver as E

pytestmark = pytest.mark.gpu


def test_api_legs():
    import zstdmt_amd as z
    eng = z.Engine(0)
    try:
        def decode(stream):
            ro, rl, cap = E.walk_brotli_records(stream)
            out = []
            for variant in (2, 1):                                 # dec4 first / the general kernel alone
                eng.set_variant("brotli_dec", variant)
                recs, status = eng.brotli_decompress_bytes(stream, ro, rl, cap)
                assert (status == 0).all()
                out.append(b"".join(recs))
            assert out[0] == out[1]
            return out[0]
        A.check_legs("gpu", decode)
    finally:
        eng.close()
