"""gpumt_lz4_decompress_blocks_seg against gpumt_lz4_decompress_blocks on the device: the hand-built, failure and linked
cases of tests/lz4_seg.py at seg_bytes 1024 and 65536, the two variants' switches, a fixed sample of changed bytes, and one
independent 4 MiB block of the golden text at the default seg_bytes."""
import pytest

import lz4_par as P
import lz4_seg as G

pytestmark = pytest.mark.gpu

CASES = G.hand_built_single(256) + G.hand_built_single(1024) + G.failures() + G.linked_runs()
SER = {}


@pytest.fixture(scope="module")
def eng():
    import zstdmt_amd as z
    e = z.Engine(0)
    yield e
    e.close()


def serial(eng, case):
    if case["name"] not in SER:
        SER[case["name"]] = P.gpu_decode(eng, case, False)
    return SER[case["name"]]


@pytest.mark.parametrize("seg", (1024, 65536))
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_seg_equals_serial(eng, case, seg):
    promised = not case["name"].startswith(("match_below", "offset_0", "malformed", "out_cap"))
    G.check(case, serial(eng, case), G.gpu_decode(eng, case, seg), seg, at_least_two=promised)


def test_end_of_block_rules_in_a_late_segment(eng):
    seen = set()
    for case in G.end_of_block_rules():
        ser = P.gpu_decode(eng, case, False)
        G.check(case, ser, G.gpu_decode(eng, case, 1024), 1024, at_least_two=True)
        seen.add((case["name"].split("_")[1], int(ser[3][0])))
    assert seen == {("full", 0), ("full", 3), ("short", 0), ("short", 3)}


def test_the_variant_switches(eng):
    """gpumt_set_variant: "lz4_block_seg" takes 0 and 1, "lz4_seg_bytes" a power of two in 256 .. 4 MiB; anything else is
    refused and changes nothing"""
    case = G.hand_built_single(1024)[0]
    ser = serial(eng, case)
    assert eng.set_variant("lz4_block_seg", 2) == -1 and eng.set_variant("lz4_block_seg", -1) == -1
    for n in (0, 1, 128, 255, 257, 3000, 65535, (4 << 20) + 1, 8 << 20, -1024):
        assert eng.set_variant("lz4_seg_bytes", n) == -1
    assert eng.set_variant("lz4_seg_bytes", 4 << 20) == 65536            # (the default, unchanged by the refusals)
    assert eng.set_variant("lz4_seg_bytes", 256) == 4 << 20
    assert eng.set_variant("lz4_seg_bytes", 65536) == 256
    G.check(case, ser, G.gpu_decode(eng, case, 1024), 1024, at_least_two=True)     # still on after the refusals
    assert eng.set_variant("lz4_block_seg", 0) == 1
    try:
        new = G.gpu_decode(eng, case, 1024)
        P.compare(case, ser, new[:4])
        assert list(new[4]) == [0]
    finally:
        assert eng.set_variant("lz4_block_seg", 1) == 0


def test_a_sample_of_changed_bytes(eng):
    base, _ = G.flip_base()
    lo, hi = G.second_segment_input(base, 1024)
    n = len(base["stream"])
    todo = list(P.flips(base, 0, range(lo, hi))) + list(P.flips(base, 0, range(0, n, 7), masks=(0x04,)))
    assert len(todo) > 100
    verdicts = set()
    for c in todo:
        ser = P.gpu_decode(eng, c, False)
        G.check(c, ser, G.gpu_decode(eng, c, 1024), 1024)
        verdicts.add(int(ser[3][0]))
    assert verdicts == {0, 3}


def test_one_independent_4mib_block(eng):
    """the real shape: 4 MiB of the golden text as one block of a 4 MiB-block frame, 64 segments at the default
    seg_bytes -- or as many as the block's own sequence stream has cuts"""
    from golden import cases
    data = cases.text(4 << 20, 91)
    b = G.Bld(92)
    b.t = data
    b.seq(64, 17, 30)
    while b.pos + 2000 < len(data):                 # literals of the text, matches into the text so far
        b.seq(300 + len(b.seqs) % 200, min(b.pos, 1000 + 977 * (len(b.seqs) % 60)), 40 + len(b.seqs) % 300)
    spec = b.end(12)
    case = G.single("one_4mib_block", spec, want=False, blkmax=4 << 20)
    want = G.count_segments(case["stream"], 0, 65536)
    assert b.pos > 63 * 65536 and want == 64
    ser = P.gpu_decode(eng, case, False)
    assert int(ser[3][0]) == 0 and int(ser[2][0]) == b.pos
    a = int(case["runs"][0]["out_off"])
    assert bytes(ser[0][a:a + 64]) == data[:64]
    assert eng.set_variant("lz4_seg_bytes", 65536) == 65536          # the default
    new = G.gpu_decode(eng, case, 65536)
    G.check(case, ser, new, 65536, at_least_two=True)
    assert list(new[4]) == [want]
