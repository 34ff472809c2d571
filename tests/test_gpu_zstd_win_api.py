"""tests/test_emu_zstd_win_api.py's legs through the library on the device: GPUMT_ZSTD_WIN=1, unset and other text."""
import pytest

import emu_driver as E
import zstd_win_api as A

pytestmark = pytest.mark.gpu


def test_api_legs():
    import zstdmt_amd as z
    eng = z.Engine(0)
    try:
        def decode(stream):
            ro, rl = E.walk_records(stream)
            out, status = eng.decompress_bytes(stream, ro, rl, codec="zstd")
            assert (status == 0).all()
            return out
        A.check_legs("gpu", decode)
    finally:
        eng.close()
