"""Plain .lz4 frames of big blocks through LZ4MT_decompressDCtx (mt_lz4_plain.inc over gpumt_lz4_decompress_blocks_seg), on
the CPU over the emulated device: independent 256 KiB blocks, a 4 MiB block holding 1.5 MiB, linked blocks, content and
block checksums, two frames and a skippable one in one stream, frames that span batches, a damaged block -- with
GPUMT_LZ4_BLOCK_SEG=1 and without the variable: same bytes, callback sizes, counters and final error.
tests/test_gpu_lz4_plain_seg_api.py runs the same cases on the device."""
import pytest

import lz4_blocks as B
import lz4_par_api as P
import lz4_seg_api as A

NAMES = sorted(A.api_cases())


@pytest.fixture(scope="module")
def on():
    return A.run_api("emu", "1")


@pytest.fixture(scope="module")
def off():
    return A.run_api("emu", None)


@pytest.mark.parametrize("name", NAMES)
def test_same_bytes_callbacks_counters_and_error_on_and_off(on, off, name):
    A.check_on_off(on, off, name, B.ERR(B.E_LIB))


def test_only_1_turns_it_on(off):
    """the host engine takes the new call under exactly "1": any other text is as good as unset"""
    name = "independent_256k_nochecksum"
    for text in ("0", "yes", "11"):
        odd = A.run_api("emu", text, only=[name])
        assert "seg" not in odd[name]
        for key in P.KEYS:
            assert odd[name][key] == off[name][key], (text, key)
