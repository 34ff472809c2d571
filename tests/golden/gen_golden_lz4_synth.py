"""Regenerates tests/golden/lz4_synth/manifest.json: for every case of tests/lz4_synth.py's stream families (seed
SEED), the SHA-256 of its frame, the verdict of the image's liblz4 1.9.3 (LZ4F_decompress) and, when accepted, the
SHA-256 of what it decoded.  Only the manifest is committed; the tests rebuild the streams from the builder and check
their SHA-256 first.  Run in the build container:
    python tests/golden/gen_golden_lz4_synth.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4_synth as S  # noqa: E402

SEED = 1


def manifest(seed=SEED):
    cases = {}
    for name, c in sorted(S.families(seed).items()):
        ok, data = S.liblz4_decompress(c["frame"])
        e = {"frame_sha256": S.sha256(c["frame"]), "liblz4": "accept" if ok else "reject"}
        if ok:
            e["content_sha256"] = S.sha256(data)
        cases[name] = e
    return {"seed": seed, "decoder": "liblz4 1.9.3 LZ4F_decompress", "cases": cases}


if __name__ == "__main__":
    assert S.liblz4_path() is not None, "needs the image's liblz4"
    d = os.path.join(HERE, "lz4_synth")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "manifest.json"), "w") as f:
        json.dump(manifest(), f, indent=1, sort_keys=True)
        f.write("\n")
