"""gpumt_lz4_decompress_blocks_par against gpumt_lz4_decompress_blocks under the emulator: the case list of
tests/lz4_par.py (hand-built linked runs, liblz4's linked frames cut at every block boundary, tables of several runs,
damaged input), every byte of a small run's second block changed in turn, and the same under the strict emulator."""
import os
import subprocess
import sys

import pytest

import helpers as H
import lz4_par as P

CASES = P.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_par_equals_serial(case):
    P.compare(case, P.emu_decode(case, False), P.emu_decode(case, True))


def test_every_byte_of_the_second_block_changed():
    base = P.flip_base_small()
    P.compare(base, P.emu_decode(base, False), P.emu_decode(base, True))
    n = int(base["blocks"]["src_len"][1])
    seen = set()
    for c in P.flips(base, 1, range(n), masks=(0xFF, 0x04, 0x40)):
        ser = P.emu_decode(c, False)
        P.compare(c, ser, P.emu_decode(c, True))
        seen.add((int(ser[3][0]), int(ser[2][0])))
    assert len({s for s, _ in seen}) == 2 and len(seen) > 3     # accepted and rejected, several lengths


def test_a_sample_of_a_liblz4_block_changed():
    if not P.HAVE_LIBLZ4:
        pytest.skip("liblz4 not on this box")
    base = P.flip_base_liblz4()
    for c in P.flips(base, 1, range(0, 40000, 997)):
        P.compare(c, P.emu_decode(c, False), P.emu_decode(c, True))


@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_par_under_the_strict_and_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "par_equals_serial and not liblz4_ or every_byte"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and "skipped" not in p.stdout, (p.stdout + p.stderr)[-1500:]
