"""Helpers of the block-parallel linked-run tests through LZ4MT_decompressDCtx (TEST CODE ONLY): linked frames that span
several batches, decoded in a process of its own with GPUMT_LZ4_RUN_PAR on, off, or holding some other text."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import helpers as H
import lz4_synth as S
from golden import cases

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")


def api_cases():
    """name -> (stream, content or None for an error case)"""
    out = {}
    blocks = []
    for i in range(200):                 # blocks of about 4 KiB whose matches reach up to 60 000 bytes back
        lits = cases.text(1500, 300 + i)
        blocks.append(("seq", [(lits, 200 + i, 2500), (b"", min(60000, 3000 * i + 900), 300), (b"0123456789ab", 0, 0)]))
    blocks.insert(130, ("stored", cases.rnd(3000, 9)))
    out["synth_linked"] = (S.frame(blocks, csize=False, ccheck=True), S.content(blocks))
    out["synth_linked_bcheck_csize"] = (S.frame(blocks, bcheck=True), S.content(blocks))
    f, _ = out["synth_linked"]
    out["err_wrong_content_checksum"] = (f[:-1] + bytes([f[-1] ^ 0x80]), None)
    bad = list(blocks)
    bad[140] = ("seq", [(b"abc", 65535, 40), (b"", 65535, 40), (b"", 65535, 65500), (b"0123456789ab", 0, 0)])
    bad[141] = ("seq", [(b"abc", 200, 5000), (b"0123456789ab", 0, 0)])
    assert len(S.content(bad[:141])) > 100000
    out["err_block_above_its_maximum"] = (S.frame(bad, csize=False, ccheck=False), None)
    if H.liblz4_frame(b"x") is not None:
        data = cases.text(700000, 5) + bytes(70000) + cases.rnd(3000, 4) * 30
        out["liblz4_default_shape"] = (H.liblz4_frame(data, block_id=4, linked=1, content_size=0, checksum=1), data)
    return out


def _run(kind, only=None):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    L = H.bind_lz4mt(C.CDLL(path))
    res = {}
    for name, (st, _) in sorted(api_cases().items()):
        if only and name not in only:
            continue
        sys.stderr.write("CASE %s\n" % name)
        sys.stderr.flush()
        rv, out, io, stats = H.lz4mt_decompress_via(L, st, threads=2)
        res[name] = dict(rv=rv, sha=hashlib.sha256(out).hexdigest(), nout=len(out), stats=list(stats),
                         reads=[list(r) if isinstance(r, (list, tuple)) else r for r in io.reads], writes=list(io.writes))
    print(json.dumps(res))


def run_api(kind, par, batch_kb=128, only=None):
    """the cases in a process of its own; par: True / False / None (variable unset), or the text GPUMT_LZ4_RUN_PAR is to
    hold -> {case: result dict + "batches", "blocks", "par" from the trace lines; "knob": what the boundary said}"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_BATCH_KB=str(batch_kb), GPUMT_TRACE="1")
    env.pop("GPUMT_BATCH_MB", None)
    env.pop("GPUMT_LZ4_RUN_PAR", None)
    if par is not None:
        env["GPUMT_LZ4_RUN_PAR"] = par if isinstance(par, str) else "1" if par else "0"
    code = "import sys; sys.path[:0] = %r; import lz4_par_api as A; A._run(%r, %r)" % (sys.path[:4], kind, only)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    name = None
    for line in p.stderr.splitlines():
        w = line.split()
        if line.startswith("CASE "):
            name = line[5:]
        elif line.startswith("[lz4mt plain]") and name:
            res[name].update(batches=int(w[2]), blocks=int(w[4]))
        elif line.startswith("[lz4mt plain par]") and name:
            res[name]["par"] = "block-parallel" in line
    res["knob"] = [line for line in p.stderr.splitlines() if "GPUMT_LZ4_RUN_PAR=" in line]
    return res


KEYS = ("rv", "sha", "nout", "stats", "reads", "writes", "batches", "blocks")


def check_on_off(on, off, name, E_LIB):
    st, want = api_cases()[name]
    a, b = on[name], off[name]
    assert a["par"] is True and b["par"] is False
    for key in KEYS:
        assert a[key] == b[key], (name, key)
    if want is None:
        assert a["rv"] == E_LIB
    else:
        assert a["rv"] == 0 and a["nout"] == len(want) and a["sha"] == hashlib.sha256(want).hexdigest()
        assert a["stats"] == [0, len(st), len(want)]
        assert a["batches"] >= 3 and a["blocks"] > 2 * a["batches"]   # several blocks per run, several runs per frame
    assert a["batches"] >= 2
