"""The corpus of hand-built streams (tests/synthetic_streams.py) on the CPU: it reaches what it claims to (the census, conditions C1 .. C8), its bytes and the
oracle's decode of them are the pinned ones (tests/golden/synthetic_streams.json, written by tools/make_golden_synthetic_streams.py where the real reference is
built), the real reference's block decoder agrees with the oracle's on every block and rectangle of it, and taking a condition's blocks away is noticed."""
import hashlib
import json
import os

import numpy as np
import pytest

import synthetic_streams as Y
from golden_util import G
from oracle import blocked_stream as B
from oracle import stream as S

GOLDEN = os.path.join(G, "synthetic_streams.json")
_CENSUS = {}


def _census(version, oracle):
    if version not in _CENSUS:
        _CENSUS[version] = Y.census(Y.corpus(version), oracle)
    return _CENSUS[version]


@pytest.mark.parametrize("version", [1, 2])
def test_census(oracle, version):
    c = _census(version, oracle)
    print(json.dumps(c))
    Y.check_census(c, version)
    assert json.loads(json.dumps(c)) == json.load(open(GOLDEN))["census"]["version %d" % version]


@pytest.mark.parametrize("version", [1, 2])
def test_bytes_and_decodes_are_the_pinned_ones(oracle, version):
    golden = json.load(open(GOLDEN))
    assert golden["decodes_confirmed_against_the_reference_build"] is True
    streams = Y.corpus(version)
    assert [s.name for s in streams] == [k for k in golden["streams"] if k.startswith("v%d-" % version)]
    for st in streams:
        bx, by = (st.W + 7) // 8, (st.H + 7) // 8
        assert bx <= 64 and by <= 64 and Y.canonical(st), st.name
        want = golden["streams"][st.name]
        assert st.sha256() == want["stream_sha256"], st.name
        assert hashlib.sha256(Y.decoded(st, oracle).tobytes()).hexdigest() == want["decode_sha256"], st.name
        assert [st.W, st.H, st.channels, int(st.bytes.size)] == want["shape"], st.name


def test_generation_is_deterministic():
    decks = Y.Decks(np.random.default_rng(1001))
    name, W, H, ch, seed, specials = Y.V1[0]
    assert np.array_equal(Y.build_v1(name, W, H, ch, seed, decks, specials).bytes, Y.corpus(1)[0].bytes)


@pytest.fixture(scope="module")
def ref_decoder():
    """the real reference's build.  (Not conftest's `ref`: that one also skips on hosts whose RSQRTPS differs from the captured table, which the float stage needs
    and the integer decoder does not.)"""
    from oracle.bind import Ref, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref not built")
    return Ref()


@pytest.mark.ref
@pytest.mark.parametrize("version", [1, 2])
def test_reference_block_decoder_agrees(oracle, ref_decoder, version):
    """the real reference decides what these streams mean: its limg_decode_block_from_factors_3d on every block and rectangle, partial sizes included"""
    ref = ref_decoder
    for st in Y.corpus(version):
        for k, (e, x0, y0, wpx, hpx, v) in enumerate(Y.entries(st)):
            rec, shift, _, _ = S.entry_fields(e)
            facs = [np.ascontiguousarray(v[f].reshape(-1).astype(np.uint8)) for f in range(3)]
            want = ref.block_decode(wpx, hpx, st.channels, rec, facs[0], facs[1], facs[2], shift)
            assert np.array_equal(oracle.block_decode(wpx, hpx, st.channels, rec, facs[0], facs[1], facs[2], shift), want), (st.name, k, st.classes[k])
            assert np.array_equal(Y.decoded(st, oracle)[y0:y0 + hpx, x0:x0 + wpx], want), (st.name, k)


# ---- the census notices what is taken away ----
def _without(streams, keep):
    """the streams with the entries for which keep(stream, index, entry, field values) is false turned into a plain fit block of shifts (1, 2, 3): same layout rules, other bytes"""
    out = []
    for st in streams:
        parse = B.parse if st.blocked else S.parse
        hdr, table, payload = parse(st.bytes)
        table = table.copy()
        new_payload = bytearray()
        classes = list(st.classes)
        for k, (e, x0, y0, wpx, hpx, v) in enumerate(Y.entries(st)):
            _, shift, bits, o = S.entry_fields(e)
            n = wpx * hpx if st.blocked else 64
            if not keep(st, k, e, v):
                for vec in S.VECS:
                    table[k][vec] = (100, 110, 120, 130) if vec.startswith("dirA") else (0, 0, 0, 0)
                shift, bits = [1, 2, 3], [7, 6, 5]
                table[k]["shift"] = 1 | (2 << 8) | (3 << 16)
                words = b"".join(S.pack_field(np.full(n, 5, dtype=np.uint32), b) for b in bits)
                classes[k] = "fit"
            else:
                words = bytes(payload[o:o + 8 * sum(S.field_words(n, b) for b in bits)])
            table[k]["payloadWord"] = len(new_payload) // 8
            new_payload += words
        data = S.assemble(st.version, st.W, st.H, st.channels, 100, int(hdr["flags"]), table, new_payload, rectangles=len(table) if st.blocked else 0)
        out.append(Y.Stream(st.name + "-cut", st.version, st.channels, st.W, st.H, data, classes))
    return out


def _shift(e):
    sw = int(e["shift"])
    return (sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF)


def _fails(streams, version, oracle):
    try:
        Y.check_census(Y.census(streams, oracle), version)
    except AssertionError:
        return True
    return False


CUTS_V1 = {
    "C1: one triple": lambda st, k, e, v: _shift(e) != (5, 0, 7),
    "C2: one escape pattern": lambda st, k, e, v: not (_shift(e) == (8, 3, 8) and int(e["shift"]) >> 24 == 4),
    "C3: the all-max fields of 3 bits": lambda st, k, e, v: not any(s == 5 and (v[f] == 7).all() for f, s in enumerate(_shift(e))),
    "C4: the large block at position 5 of rgba groups": lambda st, k, e, v: not (st.channels == 4 and (k % 64) % 8 == 5 and st.classes[k] in Y.LARGE),
    "C4: the groups without a varying alpha lane": lambda st, k, e, v: not (st.channels == 4 and all(e[S.VECS[2 * f]][3] == e[S.VECS[2 * f + 1]][3] for f in range(3))),
    "C6: the wrapped alpha products": lambda st, k, e, v: not (st.classes[k] == "extreme" and int(e["shift"]) >> 24),
    "C7: the blocks that clamp": lambda st, k, e, v: not (st.channels == 4 and st.classes[k] in ("wild", "fit", "limit")),
    "classes: over": lambda st, k, e, v: st.classes[k] != "over",
    "classes: extreme": lambda st, k, e, v: st.classes[k] != "extreme",
    "classes: limit": lambda st, k, e, v: st.classes[k] != "limit",
}
CUTS_V2 = {
    "C8: one triple": lambda st, k, e, v: _shift(e) != (5, 0, 7),
    "C8: 3-bit fields on ragged widths": lambda st, k, e, v: not (5 in _shift(e) and st.W % 8 and int(e["ox"]) + int(e["rx"]) == (st.W + 7) // 8),
    "classes: extreme": lambda st, k, e, v: st.classes[k] != "extreme",
}


@pytest.mark.parametrize("what", list(CUTS_V1))
def test_census_notices_version_1(oracle, what):
    assert _fails(_without(Y.corpus(1), CUTS_V1[what]), 1, oracle), what


@pytest.mark.parametrize("what", list(CUTS_V2))
def test_census_notices_version_2(oracle, what):
    assert _fails(_without(Y.corpus(2), CUTS_V2[what]), 2, oracle), what


def test_cutting_nothing_changes_nothing(oracle):
    for version in (1, 2):
        for a, b in zip(_without(Y.corpus(version), lambda st, k, e, v: True), Y.corpus(version)):
            assert np.array_equal(a.bytes, b.bytes)


def test_c5_geometries():
    for version in (1, 2):
        sizes = {(s.W, s.H) for s in Y.corpus(version)}
        assert any(w % 8 == 0 and h % 8 == 0 for w, h in sizes) and any(w % 8 and h % 8 and w % 4 for w, h in sizes) and any(w % 8 == 4 for w, h in sizes)
