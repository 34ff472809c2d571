"""Helpers of the segment-parallel plain .lz4 tests through LZ4MT_decompressDCtx (TEST CODE ONLY): frames of big blocks,
independent and linked, decoded in a process of its own with GPUMT_LZ4_BLOCK_SEG=1 and without the variable."""
import json
import os
import struct
import subprocess
import sys

import helpers as H
import lz4_par_api as A
import lz4_seg as G
import lz4_synth as S
from golden import cases

EMU_DIR = A.EMU_DIR


def _blocks(sizes, linked, seed, step=(7, 20)):
    """blocks of about `sizes` bytes each; linked ones reach into the blocks before"""
    out, done = [], 0
    for k, n in enumerate(sizes):
        b = G.Bld(seed + k, done if linked else 0)
        b.t = cases.text(max(n, 140000), seed + k)
        b.seq(30, 10, 40)
        while b.pos + 2 * sum(step) < n:
            far = min(b.base + b.pos, 3000 + 611 * (len(b.seqs) % 100))
            b.seq(step[0], far if len(b.seqs) % 5 == 0 else min(b.base + b.pos, 33), step[1])
        out.append(b.end())
        done += b.pos
    return out


def api_cases():
    """name -> (stream, content or None for an error case)"""
    out = {}
    ind = _blocks([250000, 262000, 90000], False, 100)
    lnk = _blocks([260000, 255000, 120000, 70000], True, 110)
    big = _blocks([1536 * 1024], False, 120, step=(150, 260))
    c_ind, c_lnk, c_big = S.content(ind, True), S.content(lnk), S.content(big, True)
    out["independent_256k_checksum"] = (S.frame(ind, indep=True, bd=5, csize=False, ccheck=True), c_ind)
    out["independent_256k_nochecksum"] = (S.frame(ind, indep=True, bd=5, csize=False, ccheck=False), c_ind)
    out["independent_4m_holding_1m5"] = (S.frame(big, indep=True, bd=7, csize=True, ccheck=False), c_big)
    out["linked_256k_block_checksums"] = (S.frame(lnk, bd=5, csize=False, ccheck=True, bcheck=True), c_lnk)
    out["linked_256k_nochecksum"] = (S.frame(lnk, bd=5, csize=False, ccheck=False), c_lnk)
    skip = struct.pack("<II", S.SKIP_MAGIC + 3, 1000) + cases.rnd(1000, 3)
    out["two_frames_and_a_skippable"] = (out["independent_256k_checksum"][0] + skip + out["linked_256k_nochecksum"][0],
                                         c_ind + c_lnk)
    bad = list(ind)
    seqs = list(bad[1][1])
    k = next(i for i, (a, _) in enumerate(S._positions(seqs)) if a >= 3 * 65536)
    seqs[k] = (seqs[k][0], 0, seqs[k][2])                 # an offset of 0 in the block's fourth segment
    bad[1] = ("seq", seqs)
    out["err_damaged_block"] = (S.frame(bad, indep=True, bd=5, csize=False, ccheck=False), None)
    return out


def _run(kind, only=None):
    import ctypes as C
    import hashlib
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


def run_api(kind, seg, batch_kb=128, only=None):
    """the cases in a process of its own; seg: the text GPUMT_LZ4_BLOCK_SEG is to hold, None = unset -> {case: result
    dict + "batches", "blocks" and, where the trace has the line, "seg" = (blocks, segments, serial)}"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, GPUMT_BATCH_KB=str(batch_kb), GPUMT_TRACE="1")
    for k in ("GPUMT_BATCH_MB", "GPUMT_LZ4_RUN_PAR", "GPUMT_LZ4_BLOCK_SEG"):
        env.pop(k, None)
    if seg is not None:
        env["GPUMT_LZ4_BLOCK_SEG"] = seg
    code = "import sys; sys.path[:0] = %r; import lz4_seg_api as A; A._run(%r, %r)" % (sys.path[:4], kind, only)
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
        elif line.startswith("[lz4mt plain seg]") and name:
            res[name]["seg"] = (int(w[3]), int(w[6]), int(w[8]))
    return res


def check_on_off(on, off, name, E_LIB):
    import hashlib
    st, want = api_cases()[name]
    a, b = on[name], off[name]
    assert "seg" in a and "seg" not in b
    for key in A.KEYS:
        assert a[key] == b[key], (name, key)
    nblk, nseg, nser = a["seg"]
    if want is None:
        assert a["rv"] == E_LIB
    else:
        assert a["rv"] == 0 and a["nout"] == len(want) and a["sha"] == hashlib.sha256(want).hexdigest()
        assert a["stats"] == [0, len(st), len(want)]
        assert nblk == a["blocks"] and nser == 0 and nseg >= len(want) // 65536    # every block in 64 KiB segments
    if want is not None and "4m" not in name:
        assert a["batches"] >= 2                          # the frame spans batches
