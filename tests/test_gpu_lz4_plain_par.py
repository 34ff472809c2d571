"""gpumt_lz4_decompress_blocks_par against gpumt_lz4_decompress_blocks on the device: the case list of
tests/lz4_par.py and a fixed sample of changed bytes in the second block of a liblz4 frame and of a small run."""
import pytest

import lz4_par as P

pytestmark = pytest.mark.gpu

CASES = P.all_cases(device=True)


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_par_equals_serial(eng, case):
    P.compare(case, P.gpu_decode(eng, case, False), P.gpu_decode(eng, case, True))


def test_the_variant_switch(eng):
    """gpumt_set_variant("lz4_run_par"): 0 and 1 are taken, anything else is refused and changes nothing"""
    case = P.flip_base_small()
    assert eng.set_variant("lz4_run_par", 2) == -1 and eng.set_variant("lz4_run_par", -1) == -1
    assert eng.set_variant("lz4_run_par", 0) == 1
    try:
        P.compare(case, P.gpu_decode(eng, case, False), P.gpu_decode(eng, case, True))
    finally:
        assert eng.set_variant("lz4_run_par", 1) == 0


def test_a_sample_of_changed_bytes(eng):
    small = P.flip_base_small()
    n = int(small["blocks"]["src_len"][1])
    todo = list(P.flips(small, 1, range(0, n, 2)))
    if P.HAVE_LIBLZ4:
        todo += list(P.flips(P.flip_base_liblz4(), 1, range(0, 40000, 173)))
    assert len(todo) > 100
    verdicts = set()
    for c in todo:
        ser = P.gpu_decode(eng, c, False)
        P.compare(c, ser, P.gpu_decode(eng, c, True))
        verdicts.add(int(ser[3][0]))
    assert verdicts == {0, 3}
