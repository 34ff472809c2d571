"""Regenerates tests/golden/zstd_synth/manifest.json: for every case of tests/zstd_synth.py's frame families (seed
SEED), the SHA-256 of its frame, the verdict of the image's libzstd 1.4.9 (ZSTD_decompress) and, when accepted, the
SHA-256 of what it decoded.  Only the manifest is committed; the tests rebuild the frames from the builder and check
their SHA-256 first.  It asserts, for every accepted case, that libzstd's output is the builder's content(), that every
case built with a status got the verdict it was built for, and that zstd_synth.DIVERGENT is exactly the set of cases
where the two verdicts differ.  Run in the build container:
    python tests/golden/gen_golden_zstd_synth.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_synth as S  # noqa: E402

SEED = 1


def manifest(seed=SEED):
    cases, differ, wrong = {}, set(), []
    for name, c in sorted(S.families(seed).items()):
        assert len(c["content"] or b"") <= 4 << 20, name
        ok, data = S.libzstd_decompress(c["frame"])
        e = {"frame_sha256": S.sha256(c["frame"]), "libzstd": "accept" if ok else "reject"}
        if ok:
            e["content_sha256"] = S.sha256(data)
            if c["content"] is not None and data != c["content"]:
                wrong.append((name, "libzstd decodes %d bytes, the builder %d" % (len(data), len(c["content"]))))
        if c["status"] is not None and (c["status"] == S.ST_OK) != ok:
            differ.add(name)
        if ok and c["content"] is None and c["status"] is None:
            wrong.append((name, "accepted by libzstd, and the builder has no content for it"))
        cases[name] = e
    assert not wrong, wrong
    # the named divergences, no more and no fewer; each one is a case libzstd accepts and the builder refuses
    assert differ == set(S.DIVERGENT), (sorted(differ - set(S.DIVERGENT)), sorted(set(S.DIVERGENT) - differ))
    assert all(cases[n]["libzstd"] == "accept" for n in S.DIVERGENT)
    return {"seed": seed, "decoder": "libzstd %d ZSTD_decompress" % S.libzstd_version(), "cases": cases}


if __name__ == "__main__":
    assert S.libzstd_decompress(b"") is not None, "needs the image's libzstd"
    d = os.path.join(HERE, "zstd_synth")
    os.makedirs(d, exist_ok=True)
    m = manifest()
    with open(os.path.join(d, "manifest.json"), "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
