"""Helpers of the block-parallel execute stage tests through ZSTDCB_decompressDCtx (TEST CODE ONLY): the committed plain
streams, a concatenation of two of them with a skippable frame between, and a wrong content checksum, decoded in a process of
its own with GPUMT_ZSTD_RUN_PAR=1 or unset; and the device boundary called directly with the variable holding other text."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import helpers as H
import zstd_blocks as Z
import zstd_pre as P

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")


def api_cases():
    """name -> (stream, content or None for an error case)"""
    out = {n: Z.fixture(n) for n in P.FIXTURE_NAMES}
    (a, wa), (b, wb) = out["l1_chk_size"], out["l19_tiled"]
    skip = struct.pack("<II", 0x184D2A53, 11) + b"skip me, ok"
    out["multi_skippable"] = (a + skip + b, wa + wb)
    out["err_wrong_checksum"] = (b[:-1] + bytes([b[-1] ^ 0x80]), None)
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


def run_api(kind, par, batch_kb, only=None):
    """the cases in a process of its own; par: True (GPUMT_ZSTD_RUN_PAR=1), None (unset) or the text it is to hold ->
    {case: result dict + "batches", "blocks", "pre_seq" from the trace lines; "knob": what the boundary said}"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_BATCH_KB=str(batch_kb), GPUMT_TRACE="1")
    for k in ("GPUMT_BATCH_MB", "GPUMT_ZSTD_RUN_PRE", "GPUMT_ZSTD_RUN_PAR"):
        env.pop(k, None)
    if par is not None:
        env["GPUMT_ZSTD_RUN_PAR"] = par if isinstance(par, str) else "1"
    code = "import sys; sys.path[:0] = %r; import zstd_par_api as A; A._run(%r, %r)" % (sys.path[:4], kind, only)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    name = None
    for line in p.stderr.splitlines():
        w = line.split()
        if line.startswith("CASE "):
            name = line[5:]
            res[name].update(batches=0, blocks=0, pre_seq=0)
        elif line.startswith("[zstdmt plain]") and name:
            res[name]["batches"] += int(w[2])
        elif line.startswith("[zstdmt plain pre]") and name:
            res[name]["blocks"] += int(w[3])
            res[name]["pre_seq"] += int(w[7])
    res["knob"] = [line for line in p.stderr.splitlines() if "GPUMT_ZSTD_RUN_PAR=" in line]
    return res


def _boundary():
    """child process: gpumt_zstd_decompress_blocks_par of the emulated boundary on one hand-built frame, with whatever
    GPUMT_ZSTD_RUN_PAR holds -> json(status, run_len, sha of the bytes, par list)"""
    import numpy as np
    import emu_driver as E
    import zstd_par as R
    from zstdmt_amd.device import ZSTD_CARRY_BYTES
    info = R.hand("back_1_2_3")[2]
    s, b, r, o = Z.tables(info, 0, 5)
    L = E.lib()
    sbuf = np.frombuffer(bytes(s) + b"\xEE" * 320, np.uint8).copy()
    area, cy = np.full(o + 64, 0xCC, np.uint8), np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8)
    rl, st, mk, pr = (np.full(n, 0xA5A5A5A5, np.uint32) for n in (1, 1, 5, 5))
    L.gpumt_zstd_decompress_blocks_par.restype = C.c_int
    sz = C.c_size_t
    rc = L.gpumt_zstd_decompress_blocks_par(C.c_void_p(1), E._p(sbuf), sz(len(s)), E._p(b), sz(5), E._p(r), sz(1), E._p(area),
                                            sz(o), E._p(cy), E._p(rl), E._p(st), E._p(mk), E._p(pr), C.c_int(0))
    n = int(rl[0])
    print(json.dumps(dict(rc=rc, st=int(st[0]), n=n, sha=hashlib.sha256(area[:n].tobytes()).hexdigest(),
                          par=[int(x) for x in pr], mark=[int(x) for x in mk])))


def run_boundary(text):
    """-> (result dict, lines the boundary wrote about the variable); text None: unset"""
    env = dict(os.environ)
    env.pop("GPUMT_ZSTD_RUN_PAR", None)
    env.pop("GPUMT_ZSTD_RUN_PRE", None)
    if text is not None:
        env["GPUMT_ZSTD_RUN_PAR"] = text
    code = "import sys; sys.path[:0] = %r; import zstd_par_api as A; A._boundary()" % (sys.path[:4],)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    return json.loads(p.stdout.strip().splitlines()[-1]), [x for x in p.stderr.splitlines() if "GPUMT_ZSTD_RUN_PAR=" in x]
