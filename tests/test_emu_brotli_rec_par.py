"""The span index of gpumt_brotli_compress_batch_index and gpumt_brotli_decompress_batch_par under the emulator: own
indexed streams of every table tier and data kind decode span by span to the serial call's results and are read by every
other decoder; one-block and empty records carry no index; foreign flushed streams with a correct index, tampered indexes
and window-encoded records with a hand-made index all come out as the serial call's, with nothing written outside a
record's output area; mixed batches, the span minimum, slices and refused scratch.

tests/test_gpu_brotli_rec_par.py runs the same cases on the device with its own `encode`, `serial` and `par` fixtures."""
import functools
import os
import subprocess
import sys

import pytest

import brotli_rec as R
import helpers as H
from golden import cases


@pytest.fixture(scope="module")
def encode():
    return functools.lru_cache(maxsize=None)(R.emu_encode)


@pytest.fixture(scope="module")
def serial():
    return R.emu_serial


@pytest.fixture(scope="module")
def par():
    return R.emu_par


def batch_of(records):
    return R.Batch([R.payload_of(r) for r in records])


# ---- 1. own streams ---------------------------------------------------------------------------------------------------------
def own(encode, serial, par, data, chunk, q):
    recs, plain = encode(data, chunk, q), encode(data, chunk, q, index=False)
    assert len(recs) == len(plain) == max(1, -(-len(data) // chunk))
    for k, (r, p) in enumerate(zip(recs, plain)):
        part = data[k * chunk:(k + 1) * chunk]
        nblk = -(-len(part) // R.BLOCK)
        payload, entries = R.split_index(R.payload_of(r)[0])
        if nblk < 2:
            assert entries is None and r == p                       # byte for byte the non-index call's
            continue
        # the same blocks, one span each, the index in front of the closing byte; the hint unchanged
        assert payload == R.payload_of(p)[0] and r[12:16] == p[12:16]
        assert [o for _, o in entries] == [min(R.BLOCK, len(part) - b * R.BLOCK) for b in range(nblk)]
        assert len(r) - len(p) == R.index_bytes(nblk) <= 8 * nblk + 13
        R.other_decoders(r, part)
    b = batch_of(recs)
    ref, got = R.check(b, serial, par)
    assert list(ref.status) == [0] * len(b) and b"".join(got.bytes_of(i) for i in range(len(b))) == data
    want = [1 if len(data[k * chunk:(k + 1) * chunk]) > R.BLOCK else 0 for k in range(len(b))]
    assert list(got.rec_par) == want
    assert got.stats["par"] == sum(want) and got.stats["fallback"] == 0
    return got


@pytest.mark.parametrize("q", R.QUALITIES, ids=lambda q: "Q%d" % q)
@pytest.mark.parametrize("size", sorted(R.SIZES))
def test_own_text(encode, serial, par, size, q):
    """text in the first and the last block of every size, R.light between them (what the emulator can afford)"""
    n = R.SIZES[size]
    data = cases.text(R.BLOCK, 40 + q) + R.light(n - R.BLOCK, 50 + q)
    if n > 2 * R.BLOCK:
        data = data[:n - 70000] + cases.text(70000, 60 + q)
    got = own(encode, serial, par, data, 2 << 20, q)
    assert got.stats["spans"] == -(-n // R.BLOCK)


@pytest.mark.parametrize("kind", sorted(R.kinds()))
def test_own_kinds(encode, serial, par, kind):
    """zeros, random (uncompressed meta-blocks), and blocks that alternate between text, random and zeros"""
    q = {"text": 5, "zeros": 1, "random": 9, "alternating": 1}[kind]
    own(encode, serial, par, R.kinds()[kind], 1 << 20, q)


def test_several_records_and_a_short_last_one(encode, serial, par):
    """chunk 256 KiB over 640 KiB: two records of two spans and one of one block, which has no index"""
    got = own(encode, serial, par, R.kinds()["alternating"], 2 * R.BLOCK, 5)
    assert list(got.rec_par) == [1, 1, 0]


@pytest.mark.parametrize("q", R.QUALITIES, ids=lambda q: "Q%d" % q)
def test_one_block_and_empty_records_have_no_index(encode, serial, par, q):
    for data in (cases.text(R.BLOCK, 3), b"", b"x"):
        recs = encode(data, 1 << 20, q)
        assert recs == encode(data, 1 << 20, q, index=False)
        _, got = R.check(batch_of(recs), serial, par)
        assert list(got.rec_par) == [0] and got.bytes_of(0) == data
    assert encode(b"", 1 << 20, q)[0][16:] == b"\x33"


# ---- 2. foreign streams -----------------------------------------------------------------------------------------------------
def test_foreign_streams(serial, par):
    """flushed libbrotli streams with a correct index: byte-aligned spans whose matches and distance codes reach back.
    Whatever the span stage makes of them, the results are the serial call's; the manifest records which are kept"""
    names = sorted(R.foreign())
    recs = []
    for name in names:
        st, spans, data, m = R.foreign()[name]
        idx = R.with_index(st, spans)
        assert H.oracle_brotli_decompress(idx, len(data) + 64) == data
        recs += [(idx, len(data)), (st, len(data) + 100)]
    ref, got = R.check(R.Batch(recs), serial, par)
    assert list(ref.status) == [0] * len(recs)
    for k, name in enumerate(names):
        data, m = R.foreign()[name][2:]
        assert got.bytes_of(2 * k) == got.bytes_of(2 * k + 1) == data
        print(name, "kept" if got.rec_par[2 * k] else "not kept")
        assert bool(got.rec_par[2 * k]) == m["kept"] and got.rec_par[2 * k + 1] == 0  # (the record of the manifest)
    assert got.stats["par"] == len(names)


# ---- 3. tampered indexes ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _victims(encode):
    """two intact indexed records of four and five spans (R.light: the emulator decodes them in a second)"""
    return [R.payload_of(r) for r in encode(R.light(3 * R.BLOCK + 500, 70), 1 << 20, 1) + encode(R.light(5 * R.BLOCK, 75), 1 << 20, 5)]


def test_tampered_indexes(encode, serial, par):
    """every damaged record between intact ones, all in one batch"""
    (good, cap), (other, ocap) = _victims(encode)
    t = R.tampered(good)
    names = sorted(t)
    recs = [(good, cap)]
    for name in names:
        recs += [(t[name], cap), (other, ocap)]
    ref, got = R.check(R.Batch(recs), serial, par)
    for k, name in enumerate(names):
        i = 1 + 2 * k
        print("%-22s status %d kept %d" % (name, ref.status[i], got.rec_par[i]))
        assert got.rec_par[i + 1] == 1
    assert got.rec_par[0] == 1
    by = {name: (int(ref.status[1 + 2 * k]), int(got.rec_par[1 + 2 * k])) for k, name in enumerate(names)}
    # the index only: the stream itself is sound, the record decoders decode it
    for name in ("comp+1", "comp-1", "comp_shifted", "out+1", "out-1", "out_shifted", "n+1", "n-1", "entry_dropped",
                 "entry_added", "magic", "comp_past_record", "comp_huge", "swapped", "zero_comp", "zero_out"):
        assert by[name] == (R.ST_OK, 0), name
    for name in ("truncated", "truncated_in_span", "last_byte"):
        assert by[name][0] != R.ST_OK and by[name][1] == 0, name


@pytest.mark.parametrize("slack", [0, -1, -R.BLOCK])
def test_capacity_below_the_sum(encode, serial, par, slack):
    """sum out_bytes above out_cap: not eligible (slack 0: exactly the capacity, kept)"""
    (good, cap), (other, ocap) = _victims(encode)
    n = sum(o for _, o in R.split_index(good)[1])
    ref, got = R.check(R.Batch([(other, ocap), (good, n + slack), (other, ocap)]), serial, par)
    assert list(got.rec_par) == [1, 1 if slack == 0 else 0, 1]
    assert ref.status[1] == (R.ST_OK if slack == 0 else R.ST_SIZE_MISMATCH)


def test_window_record_with_a_hand_made_index(encode, serial, par):
    """the window encoder's matches cross blocks: with an index over its meta-blocks the spans refuse"""
    data = cases.rnd(R.BLOCK, 61) * 3                                # noise: block 0 is stored, the later ones repeat it
    rec = encode(data, 1 << 20, 9, win=True)[0]
    payload, cap = R.payload_of(rec)
    assert R.split_index(payload)[1] is None and len(payload) < R.BLOCK + 1000
    # its meta-blocks are byte-aligned like the table encoders'.  Find the cuts by decoding prefixes: one that ends on a
    # meta-block boundary, + 0x03, decodes to whole blocks (the stored block is skipped, the other two are a few bytes)
    cuts, at = [], 0
    for k in range(1, 3):
        lo = max(at + 1, R.BLOCK)
        while H.oracle_brotli_decompress(payload[:lo] + b"\x03", len(data) + 64) != data[:k * R.BLOCK]:
            lo += 1
            assert lo < len(payload)
        cuts.append(lo - at)
        at = lo
    entries = [(cuts[0], R.BLOCK), (cuts[1], R.BLOCK), (len(payload) - 1 - at, R.BLOCK)]
    idx = R.with_index(payload, entries)
    assert H.oracle_brotli_decompress(idx, len(data) + 64) == data
    (good, gcap) = _victims(encode)[0]
    ref, got = R.check(R.Batch([(good, gcap), (idx, cap), (good, gcap)]), serial, par)
    assert list(ref.status) == [0, 0, 0] and got.bytes_of(1) == data
    assert list(got.rec_par) == [1, 0, 1] and got.stats["par"] == 3


# ---- 4. mixed batches, knobs ------------------------------------------------------------------------------------------------
def _mixed(encode):
    (good, cap), (other, ocap) = _victims(encode)
    t = R.tampered(good)
    recs = [(good, cap), (other, ocap)]
    for name in ("b_text_3000_l1", "b_mixed_l1", "b_english_l11", "b_empty"):   # written by the reference
        with open(os.path.join(H.GOLDEN_DIR, "brotli", name + ".brmt"), "rb") as f:
            recs += [R.payload_of(r) for r in R.records_of(f.read())]
    recs += [R.payload_of(encode(cases.text(20000, 5), 1 << 20, 5)[0]), (t["bit_in_span_1"], cap), (t["comp+1"], cap),
             (t["truncated"], cap), (good, cap)]
    two = R.payload_of(encode(R.light(R.BLOCK + 1, 41), 2 << 20, 1)[0])
    return recs + [two], len(R.split_index(good)[1]), len(R.split_index(other)[1])


def test_mixed_batch(encode, serial, par):
    recs, n_good, n_other = _mixed(encode)
    b = R.Batch(recs)
    _, whole = R.check(b, serial, par)
    assert whole.rec_par[0] == whole.rec_par[1] == whole.rec_par[-2] == whole.rec_par[-1] == 1
    assert n_good == 4 and n_other == 5
    _, some = R.check(b, serial, par, min_spans=5)                   # above the four-span and the two-span records
    assert some.rec_par[1] == 1 and some.rec_par[0] == some.rec_par[-2] == some.rec_par[-1] == 0
    assert some.stats["par"] == 1 and some.stats["spans"] == 5
    _, none = R.check(b, serial, par, min_spans=6)
    assert int(sum(none.rec_par)) == 0 and none.stats["par"] == 0 and none.stats["fallback"] == 0


def test_scratch_refused(encode, serial, par, request):
    """the call's own scratch above the cap: the whole batch is the serial call's, nothing is kept"""
    recs, _, _ = _mixed(encode)
    on_device = "gpu" in request.keywords
    if on_device:                                                    # the cap is in MiB there: 36 bytes per record, above 1 MiB
        recs = recs + [(R.payload_of(encode(b"tiny", 1 << 20, 1)[0])[0], 16)] * 30000
    b = R.Batch(recs)
    _, got = R.check(b, serial, par, cap=1 if on_device else len(b) * 36 + 100)
    assert int(sum(got.rec_par)) == 0 and got.stats == dict(records=len(b), par=0, spans=0, kept=0, fallback=1)
    _, got = R.check(b, serial, par)
    assert got.stats["fallback"] == 0 and got.stats["kept"] >= 4


def test_switch_off(encode, serial, par):
    recs, _, _ = _mixed(encode)
    _, got = R.check(R.Batch(recs), serial, par, rec_par=0)
    assert int(sum(got.rec_par)) == 0 and got.stats["par"] == 0 and got.stats["fallback"] == 0


# ---- 5. the emulator alone --------------------------------------------------------------------------------------------------
def test_slices(encode):
    """slices of at most six spans: records of four, five and two spans, and one of five that is a slice of its own"""
    recs, _, _ = _mixed(encode)
    b = R.Batch(recs)
    whole = R.emu_par(b)
    for slice_spans in (1, 6):
        got = R.emu_par(b, slice_spans=slice_spans)
        assert list(got.rec_par) == list(whole.rec_par) and list(got.status) == list(whole.status)
        assert list(got.out_len) == list(whole.out_len) and (got.area == whole.area).all()


def test_general_kernel_as_the_record_decoder(encode, monkeypatch):
    monkeypatch.setenv("EMU_BROTLI_DEC", "1")
    recs, _, _ = _mixed(encode)
    R.check(R.Batch(recs), R.emu_serial, R.emu_par)


@pytest.mark.parametrize("env", [{"EMU_STRICT": "1"}, {"EMU_REVERSE": "2"}], ids=["strict", "shuffled"])
def test_under_the_strict_and_shuffled_emulator(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "tampered or mixed_batch or foreign or alternating or (own_text and Q1 and 640k)"]
    p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=3000, cwd=H.ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and "skipped" not in p.stdout, (p.stdout + p.stderr)[-1500:]
