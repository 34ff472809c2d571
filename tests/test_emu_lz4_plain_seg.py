"""gpumt_lz4_decompress_blocks_seg against gpumt_lz4_decompress_blocks under the emulator: lz4_par's case list, hand-built
independent blocks whose features sit on segment cuts, failures in a later segment, linked runs of long blocks, changed
bytes, liblz4's frames -- bytes, lengths, verdicts and block_seg -- and the same under the strict and the shuffled
emulator."""
import os
import subprocess
import sys

import pytest

import helpers as H
import lz4_par as P
import lz4_seg as G

PAR_CASES = P.all_cases()
SINGLE = G.hand_built_single(256) + G.hand_built_single(1024)
FAIL = G.failures()
LINKED = G.linked_runs()
SER = {}


def serial(case):
    """the serial call's results, once per case and left unchanged"""
    if case["name"] not in SER:
        SER[case["name"]] = P.emu_decode(case, False)
    return SER[case["name"]]


def ids(cs):
    return [c["name"] for c in cs]


@pytest.mark.parametrize("seg", (65536, 1024))
@pytest.mark.parametrize("case", PAR_CASES, ids=ids(PAR_CASES))
def test_par_cases(case, seg):
    G.check(case, serial(case), G.emu_decode(case, seg), seg)


@pytest.mark.parametrize("seg", G.SEGS)
@pytest.mark.parametrize("case", SINGLE, ids=ids(SINGLE))
def test_single_block(case, seg):
    G.check(case, serial(case), G.emu_decode(case, seg), seg, at_least_two=True)


def test_single_block_cases_have_segments():
    """the cases above are no longer than 64 KiB, so at 65536 they are the serial code's; at their design size every
    valid one has several segments"""
    for d in (256, 1024):
        for case in G.hand_built_single(d):
            ser = serial(case)
            bs = G.emu_decode(case, d)[4]
            if int(ser[3][0]) == 0:
                assert int(bs[0]) >= 2, case["name"]
            assert list(G.emu_decode(case, 65536)[4]) == [0]


def test_end_of_block_rules_in_a_late_segment():
    seen = set()
    for case in G.end_of_block_rules():
        ser = P.emu_decode(case, False)
        G.check(case, ser, G.emu_decode(case, 1024), 1024, at_least_two=True)
        seen.add((case["name"].split("_")[1], int(ser[3][0])))
    assert seen == {("full", 0), ("full", 3), ("short", 0), ("short", 3)}


@pytest.mark.parametrize("case", FAIL, ids=ids(FAIL))
def test_failure_in_a_later_segment(case):
    G.check(case, serial(case), G.emu_decode(case, 1024), 1024)


@pytest.mark.parametrize("seg", G.SEGS)
@pytest.mark.parametrize("case", LINKED, ids=ids(LINKED))
def test_linked_run(case, seg):
    new = G.emu_decode(case, seg)
    G.check(case, serial(case), new, seg, at_least_two=True)
    assert all(int(x) >= 1 for x in new[4])


def test_every_second_byte_of_the_second_segment_changed():
    base, _ = G.flip_base()
    G.check(base, P.emu_decode(base, False), G.emu_decode(base, 1024), 1024, at_least_two=True)
    lo, hi = G.second_segment_input(base, 1024)
    assert hi - lo > 60
    seen = set()
    for c in P.flips(base, 0, range(lo, hi, 2)):
        ser = P.emu_decode(c, False)
        G.check(c, ser, G.emu_decode(c, 1024), 1024)
        seen.add(int(ser[3][0]))
    assert seen == {0, 3}


def test_switched_off_is_the_serial_call():
    case = SINGLE[0]
    new = G.emu_decode(case, 256, on=0)
    P.compare(case, serial(case), new[:4])
    assert list(new[4]) == [0]


@pytest.mark.parametrize("seg", (65536, 4096))
def test_liblz4_frames(seg):
    if not P.HAVE_LIBLZ4:
        pytest.skip("liblz4 not on this box")
    for case in G.liblz4_cases():
        new = G.emu_decode(case, seg)
        G.check(case, P.emu_decode(case, False), new, seg, at_least_two=True)
        assert max(int(x) for x in new[4]) == 262144 // seg


@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_seg_under_the_strict_and_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "(par_cases and not liblz4_) or single_block or end_of_block or failure_in or linked_run or every_second"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and "skipped" not in p.stdout, (p.stdout + p.stderr)[-1500:]
