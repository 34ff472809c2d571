"""Helpers of the block-run plain .zst tests (TEST CODE ONLY): a zstd frame split into the block table and run list
gpumt_zstd_decompress_blocks takes, the emulated kernels over them, hand-built frames, the committed fixtures, and a
runner that drives ZSTDCB_decompressDCtx in a process of its own (the batch size is read once per process)."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np

import helpers as H
from zstdmt_amd.device import ZSTD_BLOCK, ZSTD_RUN, XXH32_JOB, ZRUN_FIRST, ZRUN_LAST, ZSTD_CARRY_BYTES, XXH64_STATE_WORDS

EMU_DIR = os.path.join(H.ROOT, "tests", "emu")
FIX_DIR = os.path.join(H.GOLDEN_DIR, "zstd_plain")
ERR = lambda e: C.c_size_t(-e).value  # noqa: E731
E_LIB = 9          # ZSTDCB_error_compression_library (init_missing sits at 2)
ST_BAD_BLOCK = 3
MAGIC = bytes([0x28, 0xB5, 0x2F, 0xFD])


# ---- frames -------------------------------------------------------------------------------------------------------------
def walk(fr: bytes):
    """frame -> dict(window, block_max, cchk, csize (None if absent), blocks [dict(type, raw, cap, lit_type, modes)],
    expect, end); raw is the block with its 3-byte header, cap what it decodes to at most"""
    assert fr[:4] == MAGIC
    fhd = fr[4]
    single, fcs, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    at, window = 5, None
    if not single:
        wd = fr[at]
        base = 1 << (10 + (wd >> 3))
        window = base + (base >> 3) * (wd & 7)
        at += 1
    at += (0, 1, 2, 4)[did]
    n = ((1 if single else 0), 2, 4, 8)[fcs]
    csize = None
    if n:
        csize = int.from_bytes(fr[at:at + n], "little") + (256 if fcs == 1 else 0)
        at += n
    if single:
        window = csize
    info = dict(window=window, block_max=min(window, 131072), cchk=bool(fhd & 4), csize=csize, blocks=[], expect=None)
    for ent in H.zstd_walk_blocks(fr):
        tot = 3 + (1 if ent["type"] == 1 else ent["size"])
        info["blocks"].append(dict(type=ent["type"], raw=fr[at:at + tot],
                                   cap=info["block_max"] if ent["type"] == 2 else ent["size"],
                                   lit_type=ent.get("lit_type"), modes=ent.get("modes")))
        at += tot
    if info["cchk"]:
        info["expect"] = struct.unpack_from("<I", fr, at)[0]
        at += 4
    info["end"] = at
    return info


def tables(info, lo, hi, hist=0, carry=0):
    """blocks [lo, hi) of the frame as one run behind `hist` bytes of history -> (stream, ZSTD_BLOCK[n], ZSTD_RUN[1],
    out_bytes)"""
    blocks = np.zeros(hi - lo, ZSTD_BLOCK)
    stream, cap = bytearray(), 0
    for i, b in enumerate(info["blocks"][lo:hi]):
        blocks[i] = (len(stream), len(b["raw"]), info["block_max"])
        stream += b["raw"]
        cap += b["cap"]
    runs = np.zeros(1, ZSTD_RUN)
    flags = (ZRUN_FIRST if lo == 0 else 0) | (ZRUN_LAST if hi == len(info["blocks"]) else 0)
    runs[0] = (hist, cap, hist, 0, hi - lo, flags, carry)
    return bytes(stream), blocks, runs, hist + cap


def emu_decode_blocks(stream, blocks, runs, out_bytes, history=b"", carry=None):
    """emu_zstd_decompress_blocks with Engine.zstd_decompress_blocks's shape -> (output area, run_len, status, carry)"""
    import emu_driver as E
    L = E.lib()
    nblk, nrun = len(blocks), len(runs)
    sbuf = np.frombuffer(bytes(stream) + b"\xEE" * 320, np.uint8).copy()
    area = np.full(out_bytes + 64, 0xCC, np.uint8)
    area[:len(history)] = np.frombuffer(history, np.uint8)
    cy = np.full(2 * ZSTD_CARRY_BYTES, 0xA5, np.uint8) if carry is None else np.frombuffer(carry, np.uint8).copy()
    rl, st = np.full(nrun, 0xA5A5A5A5, np.uint32), np.full(nrun, 99, np.uint32)
    blocks, runs = np.ascontiguousarray(blocks, ZSTD_BLOCK), np.ascontiguousarray(runs, ZSTD_RUN)
    L.emu_zstd_decompress_blocks(E._p(sbuf), C.c_uint64(len(stream)), E._p(blocks), C.c_uint32(nblk), E._p(runs),
                                 C.c_uint32(nrun), E._p(area), C.c_uint64(out_bytes), E._p(cy), E._p(rl), E._p(st))
    assert (area[out_bytes:] == 0xCC).all(), "decoder wrote past the end of its output"
    return area[:out_bytes].tobytes(), rl, st, cy.tobytes()


def decode_cut(decode, info, cut):
    """the frame as two runs, blocks [0, cut) and [cut, n), the second behind the first one's output as history and its
    carry -> (content, status of both runs)"""
    n = len(info["blocks"])
    s1, b1, r1, o1 = tables(info, 0, cut)
    out1, rl1, st1, cy = decode(s1, b1, r1, o1)
    n1 = int(rl1[0])
    if int(st1[0]) != 0:
        return out1[:n1], [int(st1[0]), None]
    hist = min(n1, info["window"])
    s2, b2, r2, o2 = tables(info, cut, n, hist=hist)
    out2, rl2, st2, _ = decode(s2, b2, r2, o2, history=out1[n1 - hist:n1], carry=cy)
    return out1[:n1] + out2[hist:hist + int(rl2[0])], [int(st1[0]), int(st2[0])]


def cut_kinds(info):
    """{cut index: set of what the block behind the cut takes from the blocks before it}"""
    out = {}
    for k, b in enumerate(info["blocks"]):
        kinds = set()
        if b["type"] == 2:
            if b["lit_type"] == 3:
                kinds.add("treeless")
            if b["modes"] is not None:
                for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
                    if (b["modes"] >> sh) & 3 == 3:
                        kinds.add("repeat_" + name)
        elif b["type"] == 0:
            kinds.add("raw" if len(b["raw"]) > 3 else "empty")
        else:
            kinds.add("rle")
        if k:
            out[k] = kinds
    return out


def frame_of(blocks, window_log=17, csize=None, checksum=None):
    """hand-built frame: blocks = [("raw", bytes) | ("rle", byte, n) | ("cooked", block bytes with header, last bit
    ignored)] -> frame bytes; window 2^window_log, optional 8-byte content size, optional checksum value"""
    fhd = (3 << 6 if csize is not None else 0) | (4 if checksum is not None else 0)
    out = bytearray(MAGIC + bytes([fhd, (window_log - 10) << 3]))
    if csize is not None:
        out += struct.pack("<Q", csize)
    for i, b in enumerate(blocks):
        last = 1 if i == len(blocks) - 1 else 0
        if b[0] == "raw":
            out += (last | 0 << 1 | len(b[1]) << 3).to_bytes(3, "little") + b[1]
        elif b[0] == "rle":
            out += (last | 1 << 1 | b[2] << 3).to_bytes(3, "little") + bytes([b[1]])
        else:
            bh = int.from_bytes(b[1][:3], "little")
            out += ((bh & ~1) | last).to_bytes(3, "little") + b[1][3:]
    if checksum is not None:
        out += struct.pack("<I", checksum)
    return bytes(out)


def match_block(lits: bytes, off: int, ml: int):
    """one compressed block: raw literals `lits`, one sequence (ll = len(lits), match length ml at offset off), RLE-mode
    tables (RFC 8878 3.1.1.3.2) -> block bytes with header (last bit clear)"""
    ll = len(lits)
    assert 16 <= ll < 64 and 3 <= ml < 35 and off >= 1
    ll_base = [16, 18, 20, 22, 24, 28, 32, 40, 48]
    ll_bits = [1, 1, 1, 1, 2, 2, 3, 3, 4]
    li = max(i for i in range(9) if ll_base[i] <= ll)
    lc, mc, oc = 16 + li, ml - 3, (off + 3).bit_length() - 1
    acc = 1
    for v, nb in ((off + 3 - (1 << oc), oc), (0, 0), (ll - ll_base[li], ll_bits[li])):
        acc = (acc << nb) | v
    sq = bytes([1, 0x54, lc, oc, mc]) + acc.to_bytes((acc.bit_length() + 7) // 8, "little")
    body = (0 | 1 << 2 | ll << 4).to_bytes(2, "little") + lits + sq      # Raw_Literals_Block, 12-bit size
    return (2 << 1 | len(body) << 3).to_bytes(3, "little") + body


# ---- the carried checksum ---------------------------------------------------------------------------------------------
def emu_xxh64_carry(data: bytes, pieces):
    """low 32 bits of XXH64 of data continued over `pieces` by the emulated carried-state kernel"""
    import emu_driver as E
    L = E.lib()
    buf = np.frombuffer(data + b"\0" * 32, np.uint8).copy()
    states = np.full(2 * XXH64_STATE_WORDS, 0xA5A5A5A5, np.uint32)
    dig, ver = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    at, xs = 0, 0
    for i, n in enumerate(pieces):
        last = i == len(pieces) - 1
        job = np.zeros(1, XXH32_JOB)
        job["off"], job["len"] = at, n
        job["flags"] = (1 if i == 0 else xs << 8) | (2 if last else (xs ^ 1) << 9)
        if not last:
            xs ^= 1
        L.emu_xxh64_carry(E._p(buf), C.c_uint64(len(data)), E._p(job), C.c_uint32(1), E._p(states), E._p(dig), E._p(ver))
        at += n
    return int(dig[0])


def xxh64_low32(data: bytes):
    return H.oracle().zo_xxh64(data, len(data), 0) & 0xFFFFFFFF


# ---- content and fixtures ---------------------------------------------------------------------------------------------
def content(n, seed):
    """text with a stretch of random bytes and of zeros in it (raw and RLE blocks among the compressed ones)"""
    from golden import cases
    return cases.text(n // 2, seed) + cases.rnd(5000, seed + 1) + bytes(7000) + cases.text(n - n // 2 - 12000, seed + 2)


def cut_text(seed):
    from golden import cases
    return cases.text(12 * 131072 - 1000, seed)


def cut_tiled(seed):
    """short stretches of one 40 KB text over and over, two random bytes between them: blocks whose sequences look alike,
    which is where libzstd writes Repeat_Mode tables"""
    from golden import cases
    n = 12 * 131072 - 1000
    unit, r = cases.text(40000, seed), cases.rnd(n // 100 + 10, seed + 1)
    out, i = bytearray(), 0
    while len(out) < n:
        at = (i * 37) % 20000
        out += unit[at:at + 180] + r[i:i + 2]
        i += 1
    return bytes(out[:n])


FIXTURES = {  # name -> (generator, length, seed, level, checksum, content size)
    "l1_plain": ("content", 400_000, 11, 1, 0, 0), "l1_chk_size": ("content", 400_000, 12, 1, 1, 1),
    "l3_plain": ("content", 700_000, 13, 3, 0, 0), "l3_chk_size": ("content", 700_000, 14, 3, 1, 1),
    "l19_plain": ("content", 900_000, 15, 19, 0, 0), "l19_chk_size": ("content", 900_000, 16, 19, 1, 1),
    "l19_tiled": ("tiled", 0, 42, 19, 1, 1),
}


def fixture_content(name):
    gen, n, seed, *_ = FIXTURES[name]
    return content(n, seed) if gen == "content" else cut_tiled(seed)


def fixture(name):
    """-> (compressed bytes as committed under tests/golden/zstd_plain, content regenerated from its seed)"""
    with open(os.path.join(FIX_DIR, name + ".zst"), "rb") as f:
        return f.read(), fixture_content(name)


def write_fixtures():
    """regenerate the committed streams with the libzstd at hand (python -c 'import zstd_blocks as Z; Z.write_fixtures()')"""
    os.makedirs(FIX_DIR, exist_ok=True)
    for name, (_, _, _, level, chk, size) in FIXTURES.items():
        fr = H.libzstd_frame(fixture_content(name), level, checksum=chk, content_size=size)
        assert len(fr) <= 512 << 10
        with open(os.path.join(FIX_DIR, name + ".zst"), "wb") as f:
            f.write(fr)


_cut_frames = None


def cut_frames():
    """name -> (frame, content) of the every-cut test: three committed streams and the tiled one, and where libzstd is
    present 1.5 MiB (12 blocks) of text and of tiled text at levels 1, 3 and 19 made live"""
    global _cut_frames
    if _cut_frames is None:
        out = {n: fixture(n) for n in ("l1_plain", "l3_chk_size", "l19_plain", "l19_tiled")}
        if H.libzstd_frame(b"x") is not None:
            for level in (1, 3, 19):
                t, r = cut_text(31), cut_tiled(42)
                out["live_text_l%d" % level] = (H.libzstd_frame(t, level), t)
                out["live_tiled_l%d" % level] = (H.libzstd_frame(r, level, checksum=1, content_size=0), r)
        _cut_frames = out
    return _cut_frames


def cut_params():
    """(frame name, cut) for every block boundary of every frame of cut_frames(); a live frame has 12 blocks"""
    out = []
    for name in CUT_NAMES:
        n = 12 if name.startswith("live_") else len(walk(fixture(name)[0])["blocks"])
        out += [(name, cut) for cut in range(1, n)]
    return out


CUT_NAMES = ["l1_plain", "l3_chk_size", "l19_plain", "l19_tiled"] + \
    (["live_%s_l%d" % (k, lv) for k in ("text", "tiled") for lv in (1, 3, 19)] if H.libzstd_frame(b"x") is not None else [])


# ---- ZSTDCB_decompressDCtx in a process of its own -------------------------------------------------------------------
def api_cases():
    """name -> (stream, content or None for an error case); the 3 MiB frames are made live where libzstd is present, the
    committed streams stand in for them otherwise (the batches are 16 KiB of input either way)"""
    out = {}
    if H.libzstd_frame(b"x") is not None:
        a, b = content(3 << 20, 21), content(3 << 20, 22)
        out["checksum"] = (H.libzstd_frame(a, 3, checksum=1), a)
        out["no_content_size"] = (H.libzstd_frame(b, 1, content_size=0), b)
        out["level19_window"] = (H.libzstd_frame(a, 19, checksum=1, content_size=0), a)
    else:
        out["checksum"], out["no_content_size"] = fixture("l3_chk_size"), fixture("l1_plain")
        out["level19_window"] = fixture("l19_plain")
    skip = b"\x5A\x2A\x4D\x18" + (40000).to_bytes(4, "little") + bytes(40000)
    (f1, c1), (f2, c2) = out["checksum"], fixture("l1_chk_size")
    out["frame_skippable_frame"] = (f1 + skip + f2, c1 + c2)
    # errors that surface after the first batch (16 KiB of input)
    f, _ = fixture("l3_chk_size")
    assert len(f) > 8 * 16384 and (f[4] >> 5) & 1 and (f[4] >> 6) == 2       # single segment, 4-byte content size at 5
    info = walk(f)
    assert all(len(b["raw"]) > 16384 for b in info["blocks"][:3])             # so every batch holds one block
    bad = bytearray(f)
    bad[9 + len(info["blocks"][0]["raw"]) + len(info["blocks"][1]["raw"]) + 5000] ^= 0x20
    out["err_flip_third_batch"] = (bytes(bad), None)
    out["err_cut_in_later_block"] = (f[:len(f) * 3 // 4], None)
    out["err_cut_in_checksum"] = (f[:-2], None)
    out["err_wrong_content_size"] = (f[:5] + bytes([f[5] ^ 1]) + f[6:], None)
    out["err_wrong_checksum"] = (f[:-1] + bytes([f[-1] ^ 0x80]), None)
    out["err_garbage_after"] = (f + b"garbage after the frame....", None)
    return out


def _run_api(kind):
    """child process: every case through ZSTDCB_decompressDCtx of the emulated (`emu`) or the real (`gpu`) library"""
    if kind == "emu":
        H.locked_make(EMU_DIR, "libzstdmt_emu_host.so", stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        path = os.path.join(EMU_DIR, "libzstdmt_emu_host.so")
    else:
        from zstdmt_amd._native import lib_path
        path = lib_path()
    L = H.bind_lz4mt(C.CDLL(path), "ZSTDCB_")
    res = {}
    for name, (st, want) in sorted(api_cases().items()):
        sys.stderr.write("CASE %s\n" % name)
        sys.stderr.flush()
        rv, out, io, stats = H.zstdmt_decompress_via(L, st, threads=2)
        res[name] = dict(rv=rv, sha=hashlib.sha256(out).hexdigest(), nout=len(out), stats=list(stats),
                         max_write=max(io.writes, default=0), reads=[list(r) for r in io.reads[:3]], n_in=len(st))
    print(json.dumps(res))


def run_api(kind):
    """-> {case: result dict + "batches" from the trace line}, with the smallest batch the knob allows (16 KiB)"""
    env = dict(os.environ, GPUMT_BATCH_KB="16", GPUMT_TRACE="1")
    env.pop("GPUMT_BATCH_MB", None)
    code = "import sys; sys.path[:0] = %r; import zstd_blocks as Z; Z._run_api(%r)" % (sys.path[:4], kind)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    name = None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line[5:]
        elif line.startswith("[zstdmt plain]") and name:
            res[name]["batches"] = int(line.split()[2])
            res[name]["trace"] = line
    return res
