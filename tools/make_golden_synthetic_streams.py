#!/usr/bin/env python3
"""Writes tests/golden/synthetic_streams.json: the sha256 of every stream of the hand-built corpus (tests/synthetic_streams.py) and of the oracle's decode of it, and
the census of each version.  CPU only.  Run where oracle/_ref is built: the decode hashes are written only after the real reference's block decoder has agreed with
the oracle's on every block and rectangle of the corpus, and the file says so."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synthetic_streams as Y  # noqa: E402
from oracle import stream as S  # noqa: E402
from oracle.bind import Oracle, Ref, ref_available  # noqa: E402


def main():
    if not ref_available():
        sys.exit("oracle/_ref is not built: the decode hashes must be confirmed against the real reference")
    oracle, ref = Oracle(), Ref()
    out = {"decodes_confirmed_against_the_reference_build": False, "streams": {}, "census": {}}
    blocks = 0
    for version in (1, 2):
        streams = Y.corpus(version)
        for st in streams:
            want = Y.decoded(st, oracle)
            for k, (e, x0, y0, wpx, hpx, v) in enumerate(Y.entries(st)):
                rec, shift, _, _ = S.entry_fields(e)
                facs = [np.ascontiguousarray(v[f].reshape(-1).astype(np.uint8)) for f in range(3)]
                got = ref.block_decode(wpx, hpx, st.channels, rec, facs[0], facs[1], facs[2], shift)
                if not np.array_equal(got, want[y0:y0 + hpx, x0:x0 + wpx]):
                    sys.exit("%s entry %d (%s): the reference decodes other pixels than the oracle" % (st.name, k, st.classes[k]))
                blocks += 1
            out["streams"][st.name] = {"shape": [st.W, st.H, st.channels, int(st.bytes.size)], "stream_sha256": st.sha256(),
                                       "decode_sha256": hashlib.sha256(want.tobytes()).hexdigest()}
        census = Y.census(streams, oracle)
        Y.check_census(census, version)
        out["census"]["version %d" % version] = census
    out["decodes_confirmed_against_the_reference_build"] = True
    out["entries_confirmed"] = blocks
    path = os.path.join(ROOT, "tests", "golden", "synthetic_streams.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, "-", blocks, "blocks and rectangles confirmed against the reference")


if __name__ == "__main__":
    main()
