"""Helpers of the pre-pass tests through ZSTDCB_decompressDCtx (TEST CODE ONLY): single frames of about 1 MiB over
batches of 64 KiB, decoded in a process of its own with the entropy pre-pass on and off (GPUMT_ZSTD_RUN_PRE)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import helpers as H
import zstd_blocks as Z

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")


def api_cases():
    """name -> (stream, content or None for an error case): the contents of the committed streams of one level, one
    behind the other, as one frame of about 1 MiB written by libzstd where it is present; the committed streams
    themselves (one frame each, 0.4 to 0.9 MiB) where it is not"""
    out = {}
    live = H.libzstd_frame(b"x") is not None
    for level in (1, 3, 19):
        names = ["l%d_plain" % level, "l%d_chk_size" % level]
        if live:
            data = b"".join(Z.fixture_content(n) for n in names)[:1 << 20]
            out["level%d" % level] = (H.libzstd_frame(data, level, checksum=1), data)
        else:
            out["level%d" % level] = Z.fixture(names[1])
    f, _ = out["level3"]
    out["err_wrong_checksum"] = (f[:-1] + bytes([f[-1] ^ 0x80]), None)
    return out


def _run(kind, only=None):
    if kind == "emu":
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    L = H.bind_lz4mt(C.CDLL(path), "ZSTDCB_")
    res = {}
    for name, (st, _) in sorted(api_cases().items()):
        if only and name not in only:
            continue
        sys.stderr.write("CASE %s\n" % name)
        sys.stderr.flush()
        rv, out, io, stats = H.zstdmt_decompress_via(L, st, threads=2)
        res[name] = dict(rv=rv, sha=hashlib.sha256(out).hexdigest(), nout=len(out), stats=list(stats),
                         reads=[list(r) if isinstance(r, (list, tuple)) else r for r in io.reads], writes=list(io.writes))
    print(json.dumps(res))


def run_api(kind, pre_on, batch_kb=64, only=None):
    """the cases (or those named in `only`) in a process of its own; pre_on: True / False, or the text GPUMT_ZSTD_RUN_PRE
    is to hold -> {case: result dict + "batches", "blocks", "pre_seq", "pre_lit" from the trace lines; "knob": what the
    boundary said about the variable}"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_BATCH_KB=str(batch_kb), GPUMT_TRACE="1",
               GPUMT_ZSTD_RUN_PRE=pre_on if isinstance(pre_on, str) else "1" if pre_on else "0")
    env.pop("GPUMT_BATCH_MB", None)
    code = "import sys; sys.path[:0] = %r; import zstd_pre_api as A; A._run(%r, %r)" % (sys.path[:4], kind, only)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    name = None
    for line in p.stderr.splitlines():
        w = line.split()
        if line.startswith("CASE "):
            name = line[5:]
        elif line.startswith("[zstdmt plain]") and name:
            res[name]["batches"] = int(w[2])
        elif line.startswith("[zstdmt plain pre]") and name:
            res[name].update(blocks=int(w[3]), pre_seq=int(w[7]), pre_lit=int(w[11]))
    res["knob"] = [line for line in p.stderr.splitlines() if "GPUMT_ZSTD_RUN_PRE=" in line]
    return res
