"""Helper of the hand-built zstd frame tests through ZSTDCB_decompressDCtx (TEST CODE ONLY): the named cases of
tests/zstd_synth.py, each as a plain .zst stream and as a zstd-mt record, and all accepted frames back to back, decoded
in a process of its own (the batch size and GPUMT_ZSTD_RUN_PRE are read once per process)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import helpers as H
import zstd_synth as S

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")


def _run(kind, seed, names, chain):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    L = H.bind_lz4mt(C.CDLL(path), "ZSTDCB_")
    cases = S.families(seed)
    streams = []
    for n in names:
        streams.append((n + "/plain", cases[n]["frame"]))
        if S.has_fcs(cases[n]["frame"]):
            streams.append((n + "/record", S.record(cases[n]["frame"])))
    streams.append(("chain/plain", b"".join(cases[n]["frame"] for n in chain)))
    res = {}
    for key, st in streams:
        sys.stderr.write("CASE %s\n" % key)
        sys.stderr.flush()
        rv, out, _, _ = H.zstdmt_decompress_via(L, st, threads=2)
        res[key] = dict(err=bool(L.ZSTDCB_isError(rv)), rv=rv, sha=hashlib.sha256(out).hexdigest(), nout=len(out))
    print(json.dumps(res))


def run_api(kind, seed, names, chain, pre=None, batch_kb=16):
    """-> {"<case>/plain" | "<case>/record" | "chain/plain": dict(err, rv, sha, nout)}; pre = what GPUMT_ZSTD_RUN_PRE
    holds (None: unset); batches of batch_kb KiB of input, so the larger frames span several"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_BATCH_KB=str(batch_kb))
    env.pop("GPUMT_BATCH_MB", None)
    env.pop("GPUMT_ZSTD_RUN_PRE", None)
    if pre is not None:
        env["GPUMT_ZSTD_RUN_PRE"] = pre
    code = "import sys; sys.path[:0] = %r; import zstd_synth_api as A; A._run(%r, %r, %r, %r)" % (
        sys.path[:4], kind, seed, list(names), list(chain))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    return json.loads(p.stdout.strip().splitlines()[-1])
