"""Plain .zst input decoded run by run, on the device: the cases of tests/test_emu_zstd_plain_blocks.py through
Engine.zstd_decompress_blocks / Engine.xxh64_carry, ZSTDCB_decompressDCtx and the command line tool, and one frame whose
content is above 2 GiB."""
import ctypes as C
import os
import struct

import pytest

import helpers as H
import zstd_blocks as Z
from test_emu_zstd_plain_blocks import (  # noqa: F401  (the same cases, with this module's fixtures)
    test_the_cut_frames_cover_every_kind_of_carried_state, test_the_oracle_decodes_the_cut_frames, test_every_cut,
    test_cuts_before_raw_rle_and_empty_last_blocks, test_match_into_the_history_and_one_byte_in_front_of_it,
    test_treeless_block_at_the_start_of_a_frame, test_table_entries_that_leave_the_buffers, test_xxh64_carried_state,
    test_one_frame_over_many_batches, test_errors_after_the_first_batch,
    test_cli_decodes_a_committed_stream_under_small_batches)

pytestmark = pytest.mark.gpu

BIN = os.path.join(H.ROOT, "zstdmt_amd", "bin")


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def decode(eng):
    return eng.zstd_decompress_blocks


@pytest.fixture(scope="module")
def xxh64(eng):
    return eng.xxh64_carry


@pytest.fixture(scope="module")
def api():
    return Z.run_api("gpu")


@pytest.fixture(scope="module")
def cli():
    return os.path.join(BIN, "zstd-mt")


class ZeroIO(H.MemIO):
    """MemIO that counts what is written and checks that it is zeros, instead of keeping it"""

    def __init__(self, data):
        super().__init__(data)
        self.nout, self.nonzero, self.biggest = 0, 0, 0
        self._wr = H.RD_FN(self._count)
        self.rdwr = H.RefRdWr(self._rd, None, self._wr, None)

    def _count(self, _arg, bufp):
        b = bufp.contents
        if C.string_at(b.buf, b.size).count(0) != b.size:
            self.nonzero += 1
        self.nout += b.size
        self.biggest = max(self.biggest, b.size)
        return 0


def test_frame_above_2_gib():
    """16 400 RLE blocks of 128 KiB behind an 8-byte content size: 66 KB of input, 2.05 GiB of zeros.  The content bound
    of such a frame is above what a whole-frame decode can address (0x7FFFFFFF)."""
    from zstdmt_amd._native import lib_path
    lib = H.bind_lz4mt(C.CDLL(lib_path()), "ZSTDCB_")
    nblk, n = 16400, 16400 * 131072
    assert n > 1 << 31
    fr = bytearray(Z.MAGIC + bytes([3 << 6, (17 - 10) << 3]) + struct.pack("<Q", n))
    fr += ((1 << 1 | 131072 << 3).to_bytes(3, "little") + b"\0") * (nblk - 1)
    fr += ((1 | 1 << 1 | 131072 << 3).to_bytes(3, "little") + b"\0")
    io = ZeroIO(bytes(fr))
    ctx = lib.ZSTDCB_createDCtx(2, 0)
    rv = lib.ZSTDCB_decompressDCtx(ctx, C.byref(io.rdwr))
    stats = (lib.ZSTDCB_GetFramesDCtx(ctx), lib.ZSTDCB_GetInsizeDCtx(ctx), lib.ZSTDCB_GetOutsizeDCtx(ctx))
    lib.ZSTDCB_freeDCtx(ctx)
    assert rv == 0, lib.ZSTDCB_getErrorString(rv)
    assert io.nout == n and io.nonzero == 0 and io.biggest <= 131072
    assert stats == (0, len(fr), n)
