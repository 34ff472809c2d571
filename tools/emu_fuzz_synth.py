"""Emulator run of tests/lz4_synth.py's hand-built stream families over a range of seeds (the suite pins seed 1):
every decoder variant -- frames + parse4 + copy3 at three ring sizes, the frame-serial kernel -- and the oracle must
give liblz4 1.9.3's verdict on every record of the lz4-mt record path, and its bytes where it accepts
(developer tool, needs the image's liblz4: python tools/emu_fuzz_synth.py [first] [last])."""
import ctypes as C
import sys
sys.path.insert(0, 'tests')
import helpers as H, emu_driver as E, lz4_synth as S
from test_emu_lz4_synth import record_path
n0 = int(sys.argv[1]) if len(sys.argv) > 1 else 2
n1 = int(sys.argv[2]) if len(sys.argv) > 2 else 12
assert S.liblz4_path(), "needs liblz4"
bad = 0
for seed in range(n0, n1):
    cases = S.families(seed)
    verdict = {n: S.liblz4_decompress(c["frame"]) for n, c in cases.items()}
    for n, c in sorted(cases.items()):
        buf = C.create_string_buffer(1 << 23)
        r = H.oracle().zo_lz4f_decompress(c["frame"], len(c["frame"]), buf, 1 << 23)
        ok, data = verdict[n]
        if (r != H.SIZE_ERR) != ok or (ok and buf.raw[:r] != data):
            bad += 1
            print("seed", seed, n, "oracle", r != H.SIZE_ERR, "liblz4", ok)
    names = [n for n in sorted(cases) if record_path(cases[n])]
    stream = b"".join(S.record(cases[n]["frame"]) for n in names)
    for v in (0 | 12 << 4, 0 | 13 << 4, 0 | 14 << 4, 1):
        out, status, oo, ol = E.decompress(stream, v, layout=True)
        for i, n in enumerate(names):
            ok, data = verdict[n]
            got = int(status[i]) == 0
            if got != ok or (ok and out[int(oo[i]):int(oo[i]) + int(ol[i])] != data):
                bad += 1
                print("seed", seed, n, "variant", v, "status", int(status[i]), "liblz4", ok)
    print("seed", seed, len(cases), "cases", flush=True)
print("mismatches:", bad)
sys.exit(1 if bad else 0)
