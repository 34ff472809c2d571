"""Regenerates tests/golden/lz4_synth/rec_manifest.json: for every hand-built frame of tests/lz4_rec.py (the records of
the block-parallel record path tests: the mixed batch, the frame-level edges, the seg route's frames), the SHA-256 of the
frame, the verdict of the image's liblz4 1.9.3 (LZ4F_decompress) and, when accepted, the SHA-256 of what it decoded.  Only
the manifest is committed; the tests rebuild the frames from the builder and check their SHA-256 first.  Run in the build
container:
    python tests/golden/gen_golden_lz4_rec.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import lz4_rec as K  # noqa: E402
import lz4_synth as S  # noqa: E402


def manifest():
    cases = {}
    for name, fr in sorted(K.manifest_frames().items()):
        ok, data = S.liblz4_decompress(fr)
        e = {"frame_sha256": S.sha256(fr), "liblz4": "accept" if ok else "reject"}
        if ok:
            e["content_sha256"] = S.sha256(data)
        cases[name] = e
    return {"decoder": "liblz4 1.9.3 LZ4F_decompress", "cases": cases}


if __name__ == "__main__":
    assert S.liblz4_path() is not None, "needs the image's liblz4"
    with open(K.REC_MANIFEST, "w") as f:
        json.dump(manifest(), f, indent=1, sort_keys=True)
        f.write("\n")
