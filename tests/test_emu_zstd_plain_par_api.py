"""The block-parallel execute stage under ZSTDCB_decompressDCtx (mt_zstd_plain.inc over gpumt_zstd_decompress_blocks_par),
on the CPU over the emulated device: the committed plain streams, a concatenation with a skippable frame between and a
wrong content checksum, over batches of 64 KiB and of 512 KiB, under GPUMT_ZSTD_RUN_PAR=1 and with the variable unset.
tests/test_gpu_zstd_plain_par_api.py runs the same cases on the device (`kind`)."""
import hashlib

import pytest

import zstd_blocks as Z
import zstd_par_api as A

BATCHES = (64, 512)


@pytest.fixture(scope="module")
def kind():
    return "emu"


@pytest.fixture(scope="module")
def runs(kind):
    return {(kb, par): A.run_api(kind, par, kb) for kb in BATCHES for par in (True, None)}


@pytest.mark.parametrize("kb", BATCHES)
@pytest.mark.parametrize("name", sorted(n for n, (_, w) in A.api_cases().items() if w is not None))
def test_same_content_trace_and_counters(runs, name, kb):
    st, want = A.api_cases()[name]
    a, b = runs[kb, True][name], runs[kb, None][name]
    assert a["rv"] == 0 and a["nout"] == len(want) and a["sha"] == hashlib.sha256(want).hexdigest()
    assert a["stats"] == [0, len(st), len(want)]
    for key in ("rv", "sha", "nout", "stats", "reads", "writes", "batches"):
        assert a[key] == b[key], key
    assert a["pre_seq"] > 0 and b["pre_seq"] == 0        # the new call ran (its marks came back), or no stage did
    if kb == 64:
        assert a["batches"] >= 3                         # the frame spans batches


@pytest.mark.parametrize("kb", BATCHES)
def test_wrong_checksum_is_refused_with_the_same_code(runs, kb):
    assert runs[kb, True]["err_wrong_checksum"]["rv"] == runs[kb, None]["err_wrong_checksum"]["rv"] == Z.ERR(Z.E_LIB)
    assert runs[kb, True]["knob"] == runs[kb, None]["knob"] == []


def test_other_text_in_the_variable(kind):
    """through the host engine anything but 1 is today's behaviour; the device boundary, called directly, says that it
    ignored the text and decodes with the stage on; 0 turns the stage off there (block_par all 0, same result)"""
    c = A.run_api(kind, "yes", 512, ["l19_tiled"])["l19_tiled"]
    assert c["rv"] == 0 and c["pre_seq"] == 0
    if kind != "emu":
        return
    on, said_on = A.run_boundary(None)
    odd, said_odd = A.run_boundary("yes")
    off, said_off = A.run_boundary("0")
    assert said_on == said_off == [] and len(said_odd) == 1 and "GPUMT_ZSTD_RUN_PAR=yes ignored" in said_odd[0]
    assert on["rc"] == 0 and on["st"] == 0 and on["par"] == [1] * 5 and odd == on
    assert off["par"] == [0] * 5 and {k: v for k, v in off.items() if k != "par"} == {k: v for k, v in on.items() if k != "par"}
