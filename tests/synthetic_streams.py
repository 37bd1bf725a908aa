"""Hand-built "LMG3" streams: a corpus of both versions made directly from (records, shift triples, field values) with the oracle's pieces (fill_entry, field_bits,
pack_field, assemble, RECT), and the census of what it reaches.  The container (include/limg_hip.h) is much wider than what a fit of byte pixels emits: any int16
record, every shift triple of {0..8}^3, every escape pattern, fields at any bit offset.  No encoder is involved; a stream's expected image is the oracle's decode of
its bytes (oracle.stream.decode / oracle.blocked_stream.decode: the reference's a16 with 32-bit wrapping products).  Not a test module.

Record classes (24 int16 values per record; classify() tells them apart from the bytes alone):
  fit      all values in [-255, 255]
  limit    every value -2700 or +2700 (kPackedLimit of k_stream_decode: the last values of the packed 16-bit form)
  over     a fit record with exactly one value at +2701 or -2701 (the first values beyond it)
  extreme  factor B carries the negated normal of A, with A's shift and A's field values, and C places the sum: values reach -32768 and 32767, normals +-65535,
           the single terms are huge and the sum lands inside 0 .. 255
  wild     uniform int16 (few: they mostly clamp)
A block is LARGE where a value lies beyond +-2700: over, extreme, wild.  Field values are not random: place() tries a few candidates per pixel and keeps the one
that puts the most channels into 1 .. 254, so that a clamp cannot hide a wrong term (census C7 holds the corpus to it).

Everything is seeded (np.random.default_rng) and deterministic; tests/golden/synthetic_streams.json pins the bytes."""
import hashlib
import itertools

import numpy as np

from oracle import blocked_stream as B
from oracle import stream as S

CLASSES = ("fit", "limit", "over", "extreme", "wild")
LARGE = ("over", "extreme", "wild")
LIMIT = 2700  # kPackedLimit (limg_amd/csrc/limg_hip_stream.hip)
MUL = np.array([1, 2, 4, 8, 17, 36, 85, 255, 256], dtype=np.int64)  # (1 << s) + decode_bias(s), src/limg_bit_crush_simd.h:611-619
TRIPLES = list(itertools.product(range(9), repeat=3))


def subsets_of(triple):
    """the escape masks a 4-channel block of this triple can carry: every subset of its shift-8 factors"""
    eights = [k for k in range(3) if triple[k] == 8]
    return [sum(1 << k for k in c) for r in range(len(eights) + 1) for c in itertools.combinations(eights, r)]


ESCAPES = [(t, m) for t in TRIPLES for m in subsets_of(t)]
assert len(TRIPLES) == 729 and len(ESCAPES) == 1000


# ---- the decoder's arithmetic in numpy (for placing field values and for the census; the EXPECTED image is always the oracle's) ----
def wrap32(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def constants(rec, shift, channels):
    """rec: (6, 4) int -> normals and additive terms (3, 4) int64 as the reference's decoder sets them up (src/limg_decode.h:40-101, 139-196)"""
    r = np.asarray(rec, dtype=np.int64)
    n, m = r[1::2] - r[0::2], r[0::2].copy()
    for f in range(3):
        if shift[f] > 7:
            n[f, :3] = 0
            if f > 0:
                m[f, :3] = 0
    if channels == 3:
        n[:, 3], m[:, 3] = 0, 0xFFFF
    return n, m


def estimate(rec, shift, channels, v):
    """v: (3, ...) field values -> (4, ...) int64: the sum of the three 32-bit terms BEFORE the clamp"""
    n, m = constants(rec, shift, channels)
    v = np.asarray(v, dtype=np.int64)
    one = (1,) * (v.ndim - 1)
    d = v * MUL[list(shift)].reshape((3,) + one)
    t = wrap32(d[:, None] * n.reshape((3, 4) + one) + (m.reshape((3, 4) + one) << 8) + 128) >> 8
    return wrap32(t.sum(axis=0))


def rec_array(e):
    """a table entry's six vectors as (6, 4) int64"""
    return np.array([e[v] for v in S.VECS], dtype=np.int64).reshape(6, 4)


def classify(rec):
    r = np.asarray(rec, dtype=np.int64).reshape(6, 4)
    a = np.abs(r)
    if a.max() <= 255:
        return "fit"
    if (a == LIMIT).all():
        return "limit"
    if (a == LIMIT + 1).sum() == 1 and (a > 255).sum() == 1:
        return "over"
    if np.array_equal(r[1] - r[0], -(r[3] - r[2])):
        return "extreme"
    return "wild"


def is_large(rec):
    return int(np.abs(np.asarray(rec, dtype=np.int64)).max()) > LIMIT


# ---- records ----
class Decks:
    """What the corpus cycles through so that every case occurs: shuffled once per corpus, drawn in turn."""

    def __init__(self, rng, rectangles=False):
        self.rng = rng
        self.triples = {3: self._cycle(TRIPLES), 4: self._cycle(TRIPLES)}
        self.escapes = self._cycle(ESCAPES)
        if rectangles:  # version 2 has fewer entries: one deck of triples for all its streams, the escape mask drawn at random
            self.triples[4], self.escapes = self.triples[3], None
        self.over = {3: self._cycle(list(itertools.product(range(24), (1, -1)))), 4: self._cycle(list(itertools.product(range(24), (1, -1))))}
        self.cancel = self._cycle(list(itertools.product(range(9), repeat=2)))  # (shift of A and B, shift of C)
        # C3: field f of b bits all zero / all max / random, and C's bound: all normals at +-5400 under all-max fields
        self.fields = [(f, b, kind) for b in range(1, 9) for f in range(3) for kind in ("zero", "max", "random")]
        self.bounds = [(s, sign) for s in (0, 7, 3) for sign in (1, -1)]

    def _cycle(self, items):
        items = list(items)
        order = self.rng.permutation(len(items))
        return itertools.cycle([items[i] for i in order])


def _escape_lane(rec, triple, mask, rng, lo, hi):
    """lane 3 of a 4-channel record under an escape mask: a shift-8 factor's alpha normal is non-zero exactly where its bit is set"""
    for f in range(3):
        if triple[f] == 8:
            if (mask >> f) & 1:
                while rec[2 * f + 1, 3] == rec[2 * f, 3]:
                    rec[2 * f + 1, 3] = rng.integers(lo, hi + 1)
            else:
                rec[2 * f + 1, 3] = rec[2 * f, 3]


def _flat_alpha(rec):
    rec[1::2, 3] = rec[0::2, 3]


def make_fit(rng, triple, mask, channels, alpha):
    rec = np.zeros((6, 4), dtype=np.int64)
    if rng.integers(8) == 0:  # anywhere in the class: these reach the clamps, both ways
        rec[:] = rng.integers(-255, 256, (6, 4))
    else:
        rec[0:2] = rng.integers(20, 236, (2, 4))
        rec[2:4] = rng.integers(-40, 41, (2, 4))
        rec[4:6] = rng.integers(-20, 21, (2, 4))
    if channels == 3:
        rec[:, 3] = rng.choice([-255, -200, -3, 7, 129, 255], 6)
    elif alpha:
        _escape_lane(rec, triple, mask, rng, -255, 255)
    else:
        _flat_alpha(rec)
    return rec, dict()


def make_limit(rng, triple, mask, channels, alpha, bound=None):
    rec = np.zeros((6, 4), dtype=np.int64)
    if bound is not None:  # every normal at +5400 (-5400): the largest terms the packed form must hold
        rec[0::2], rec[1::2] = -bound * LIMIT, bound * LIMIT
        return rec, dict(fixed={0: "max", 1: "max", 2: "max"})
    plan = dict()
    if rng.integers(16) == 0 or min(triple) == 8:
        rec[:] = rng.choice([-LIMIT, LIMIT], (6, 4))
    else:  # one pattern for all channels, so that one field value suits them all: the factor of the finest field walks from -+2700 through zero, the others' offsets cancel
        s = int(np.argmin(triple))
        o1, o2 = [f for f in range(3) if f != s]
        sg, tg = rng.choice([-1, 1], 2)
        rec[2 * s], rec[2 * s + 1] = -sg * LIMIT, sg * LIMIT
        rec[2 * o1], rec[2 * o2] = tg * LIMIT, -tg * LIMIT
        rec[2 * o1 + 1] = rec[2 * o1] * rng.choice([-1, 1])
        rec[2 * o2 + 1] = rec[2 * o2] * rng.choice([-1, 1])
        # (a shift-8 factor that is not escaped keeps its offset in the alpha lane alone: there the field suits either the colours or alpha -- alpha takes its turn)
        plan = dict(solver=s, lead=3 if channels == 4 and alpha and max(triple) == 8 and mask == 0 else int(rng.integers(3)))
    if channels == 3:
        rec[:, 3] = rng.choice([-LIMIT, LIMIT], 6)
    elif alpha:
        for f in range(3):  # a shift-8 factor's alpha normal is non-zero exactly where it is escaped
            if triple[f] == 8:
                rec[2 * f + 1, 3] = -rec[2 * f, 3] if (mask >> f) & 1 else rec[2 * f, 3]
    else:
        _flat_alpha(rec)
    return rec, plan


def make_over(rng, triple, mask, channels, alpha, where):
    """a fit record whose value `pos` (0 .. 23: vector * 4 + lane) is +-2701; its factor's field is solved for so that its channel still lands inside"""
    pos, sign = where
    rec, _ = make_fit(rng, triple, mask, channels, alpha)
    while np.abs(rec).max() > 235:  # (not the class-wide kind: the other 23 values leave room)
        rec, _ = make_fit(rng, triple, mask, channels, alpha)
    vec, lane = pos // 4, pos % 4
    f = vec // 2
    if channels == 4 and lane == 3 and (not alpha or (triple[f] == 8 and not (mask >> f) & 1)):
        lane = 0  # this alpha normal has to stay zero, which one value alone cannot: the value goes to red
    rec[vec, lane] = sign * (LIMIT + 1)
    return rec, (dict(solver=f, lead=lane) if lane < channels else dict())


def _clip16(x):
    return min(32767, max(-32768, int(x)))


def make_extreme(rng, st, ct, mask, channels, alpha):
    """shifts (st, st, ct).  Per lane: A = (a, a + n), B = (b, b - n) with a + b small, C (or, at ct == 8 where the decoder drops C's colour offset, b itself) places the
    sum.  At st == 8 the decoder drops the colour normals and B's colour offset whatever they hold: they stay huge, and a alone is small."""
    rec = np.zeros((6, 4), dtype=np.int64)
    for c in range(4):
        colour = c < 3
        target = int(rng.integers(30, 221))
        flat_ab = not colour and channels == 4 and (not alpha or (st == 8 and not mask & 1))
        flat_c = not colour and channels == 4 and (not alpha or (ct == 8 and not (mask >> 2) & 1))
        if colour and st == 8:
            a = target if ct == 8 else int(rng.integers(10, 120))
            n = int(rng.integers(-32768 - a, 32768 - a))
        elif rng.integers(3) == 0 or (not colour and st == 8):
            a, n = (-32768, 65535) if rng.integers(2) else (32767, -65535)
        else:
            a = int(rng.integers(-32768, 32768))
            n = int(rng.integers(-32768 - a, 32768 - a)) or 1
            if not -32768 <= a + n <= 32767:
                n = -n
        if flat_ab:
            n = 0
        if colour and st == 8:
            b, rest = int(rng.integers(-32768, 32768)), a
        else:
            b = -a + (target if colour and ct == 8 else int(rng.integers(-100, 101)))
        b = min(32767, 32767 + n, max(-32768, -32768 + n, b))  # b and b - n are both int16
        if not (colour and st == 8):
            rest = a + b
        rec[0, c], rec[1, c], rec[2, c], rec[3, c] = a, a + n, b, b - n
        if colour and ct == 8:
            rec[4, c], rec[5, c] = rng.integers(-32768, 32768, 2)
        else:
            off = _clip16(target - rest)
            spread = 0 if flat_c else int(rng.integers(-60, 61))
            if not colour and channels == 4 and ct == 8 and not flat_c and spread == 0:
                spread = 17
            rec[4, c], rec[5, c] = off, _clip16(off + spread)
            if rec[5, c] == off and spread:
                rec[5, c] = off - abs(spread)
    return rec, dict(tie=True, peak=st == 8)


def make_wild(rng, channels, alpha):
    rec = rng.integers(-32768, 32768, (6, 4)).astype(np.int64)
    if channels == 4 and not alpha:
        _flat_alpha(rec)
    return rec, dict(tries=1)


# ---- field values ----
def place(rng, rec, shift, bits, channels, npx, solver=None, lead=0, tie=False, fixed=None, peak=False, tries=12):
    """(3, npx) field values: `tries` candidates per pixel, the one with the most channels inside 1 .. 254 kept.  solver: the factor whose value is solved for so that
    channel `lead` lands on a random target; tie: B takes A's values; peak: every fifth value of A is the field's largest; fixed: {factor: "zero" | "max" | "random"}
    fields that are given."""
    fixed = fixed or {}
    top = [(1 << b) - 1 for b in bits]
    v = np.stack([rng.integers(0, top[f] + 1, (tries, npx)) for f in range(3)]).astype(np.int64)
    for f, kind in fixed.items():
        if kind != "random":
            v[f] = 0 if kind == "zero" else top[f]
    if peak:
        v[0][:, ::5] = top[0]
    if tie and bits[0] == bits[1]:
        v[1] = v[0]
    n, _ = constants(rec, shift, channels)
    if solver is not None and solver not in fixed and bits[solver] and n[solver, lead] != 0 and not (tie and solver < 2):
        v[solver] = 0
        base = estimate(rec, shift, channels, v)[lead]
        target = rng.integers(8, 248, (tries, npx))
        d = (target - base) * 256.0 / float(n[solver, lead])
        v[solver] = np.clip(np.rint(d / float(MUL[shift[solver]])), 0, top[solver]).astype(np.int64)
    est = estimate(rec, shift, channels, v)[:channels]
    score = ((est >= 1) & (est <= 254)).sum(axis=0)
    best = np.argmax(score, axis=0)
    return v[:, best, np.arange(npx)]


# ---- version 1 ----
class Stream:
    """name, version, channels, W, H, bytes (numpy uint8), classes (per block / rectangle, as built)"""

    def __init__(self, name, version, channels, W, H, data, classes):
        self.name, self.version, self.channels, self.W, self.H, self.bytes, self.classes = name, version, channels, W, H, data, classes

    @property
    def blocked(self):
        return self.version == 2

    def decode(self, oracle):
        return (B.decode if self.blocked else S.decode)(self.bytes, oracle)

    def sha256(self):
        return hashlib.sha256(self.bytes.tobytes()).hexdigest()


# the kinds of a group of 8 blocks (block g: unit g // 64, group (g % 64) // 8): no large block, all large, exactly one at position k
GROUP_KINDS = ["none", "all"] + ["one@%d" % k for k in range(8)]


def _group_plan(n_blocks, channels, rng):
    """per block: (large?, alpha lane may vary?).  The groups cycle through GROUP_KINDS; of a 4-channel stream every eighth round of kinds has no varying alpha lane."""
    large, alpha = np.zeros(n_blocks, dtype=bool), np.ones(n_blocks, dtype=bool)
    gi = 0
    for unit in range(0, n_blocks, 64):
        for g0 in range(unit, min(unit + 64, n_blocks), 8):
            kind = GROUP_KINDS[gi % 10]
            idx = np.arange(g0, min(g0 + 8, unit + 64, n_blocks))
            if kind == "all":
                large[idx] = True
            elif kind != "none":
                k = int(kind[4:])
                if k < len(idx):
                    large[idx[k]] = True
            if channels == 4 and (gi // 10) % 8 == 1:
                alpha[idx] = False
            gi += 1
    return large, alpha


def _spec(decks, rng, channels, large, alpha, state):
    """one block's or rectangle's (class, record, shift triple, field plan)"""
    def draw():
        if channels == 4 and alpha and decks.escapes is not None:
            return next(decks.escapes)
        triple = next(decks.triples[channels])
        return triple, (int(rng.choice(subsets_of(triple))) if channels == 4 and alpha else 0)

    if large:
        k = state["large"] = state.get("large", 0) + 1
        cls = "wild" if k % 16 == 0 else ("over" if k % 2 else "extreme")
    else:
        k = state["small"] = state.get("small", 0) + 1
        cls = "limit" if k % 3 == 0 else "fit"
    if cls == "fit":
        if state.get("fields"):
            f, b, kind = state["fields"].pop(0)
            triple = [int(rng.integers(9)) for _ in range(3)]
            triple[f] = 8 - b
            triple = tuple(triple)
            mask = int(rng.choice(subsets_of(triple))) if channels == 4 and alpha else 0
            rec, plan = make_fit(rng, triple, mask, channels, alpha)
            plan["fixed"] = {f: kind}
        else:
            triple, mask = draw()
            rec, plan = make_fit(rng, triple, mask, channels, alpha)
    elif cls == "limit":
        if state.get("bounds"):
            s, sign = state["bounds"].pop(0)
            triple, mask = (s, s, s), 0
            rec, plan = make_limit(rng, triple, mask, channels, alpha, bound=sign)
            if channels == 4 and not alpha:
                _flat_alpha(rec)
        else:
            triple, mask = draw()
            rec, plan = make_limit(rng, triple, mask, channels, alpha)
    elif cls == "over":
        triple, mask = draw()
        rec, plan = make_over(rng, triple, mask, channels, alpha, next(decks.over[channels]))
    elif cls == "extreme":
        st, ct = next(decks.cancel)
        triple = (st, st, ct)
        mask = int(rng.choice(subsets_of(triple))) if channels == 4 and alpha else 0
        if st == 8 and (mask & 3) in (1, 2):
            mask |= 3  # A and B share their field values: escaped together or not at all
        rec, plan = make_extreme(rng, st, ct, mask, channels, alpha)
    else:
        triple = next(decks.triples[channels])  # (its escapes are whatever its alpha normals say)
        rec, plan = make_wild(rng, channels, alpha)
    assert rec.min() >= -32768 and rec.max() <= 32767
    return cls, rec, triple, plan


def _entry_record(rec):
    out = np.zeros(1, dtype=S.BLOCK)[0]
    for k, v in enumerate(S.VECS):
        out[v] = rec[k]
    return out


def build_v1(name, W, H, channels, seed, decks, specials=False):
    rng = np.random.default_rng(seed)
    bx, by = (W + 7) // 8, (H + 7) // 8
    assert bx <= 64 and by <= 64
    large, alpha = _group_plan(bx * by, channels, rng)
    state = dict(fields=list(decks.fields), bounds=list(decks.bounds)) if specials else {}
    table = np.zeros(bx * by, dtype=S.BLOCK)
    payload = bytearray()
    classes = []
    for g in range(bx * by):
        cls, rec, triple, plan = _spec(decks, rng, channels, bool(large[g]), bool(alpha[g]), state)
        e = _entry_record(rec)
        bits, raw = S.field_bits(triple, e, channels)
        S.fill_entry(table[g], e, triple, raw, len(payload) // 8)
        v = place(rng, rec, triple, bits, channels, 64, **plan).reshape(3, 8, 8)
        i, j = g % bx, g // bx
        v[:, min(8, H - 8 * j):, :] = 0  # pixels outside the image are 0
        v[:, :, min(8, W - 8 * i):] = 0
        for f in range(3):
            if bits[f]:
                payload += S.pack_field(v[f], bits[f])
        classes.append(cls)
    assert not state.get("fields") and not state.get("bounds")
    data = S.assemble(S.VERSION, W, H, channels, 100, 1, table, payload)
    return Stream(name, 1, channels, W, H, data, classes)


# ---- version 2 ----
def tiling(bx, by, rng):
    """rectangles (ox, oy, rx, ry) that cover the bx x by grid exactly once: a strip along the whole top row and one down the rest of the left column, a rectangle of
    72 blocks, rectangles with rx, ry > 1 on the right and the bottom edge, and small ones (mostly single blocks) for the rest; in shuffled order"""
    free = np.ones((by, bx), dtype=bool)
    out = []

    def take(ox, oy, rx, ry):
        assert free[oy:oy + ry, ox:ox + rx].all()
        free[oy:oy + ry, ox:ox + rx] = False
        out.append((ox, oy, rx, ry))

    take(0, 0, bx, 1)
    take(0, 1, 1, by - 1)
    take(2, 2, 9, 8)
    take(bx - 3, by - 2, 3, 2)   # the clipped corner
    take(bx - 2, 3, 2, 5)        # the right edge
    take(4, by - 3, 6, 3)        # the bottom edge
    take(12, 2, 1, 7)
    take(2, 11, 11, 1)
    for oy in range(by):
        for ox in range(bx):
            if not free[oy, ox]:
                continue
            rx, ry = (1, 1) if rng.integers(10) < 6 else (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
            while not free[oy:oy + ry, ox:ox + rx].all() or ox + rx > bx or oy + ry > by:
                rx, ry = (rx - 1, ry) if rx > ry else (rx, max(1, ry - 1))
            take(ox, oy, rx, ry)
    assert not free.any()
    return [out[i] for i in rng.permutation(len(out))]


def build_v2(name, W, H, channels, seed, decks):
    rng = np.random.default_rng(seed)
    bx, by = (W + 7) // 8, (H + 7) // 8
    assert 16 <= bx <= 64 and 16 <= by <= 64
    rects = tiling(bx, by, rng)
    table = np.zeros(len(rects), dtype=B.RECT)
    payload = bytearray()
    classes, state = [], {}
    for r, (ox, oy, rx, ry) in enumerate(rects):
        large = r % 5 in (1, 3)
        alpha = r % 7 != 2
        cls, rec, triple, plan = _spec(decks, rng, channels, large, alpha, state)
        e = _entry_record(rec)
        bits, raw = S.field_bits(triple, e, channels)
        S.fill_entry(table[r], e, triple, raw, len(payload) // 8)
        table[r]["ox"], table[r]["oy"], table[r]["rx"], table[r]["ry"] = ox, oy, rx, ry
        _, _, wpx, hpx = B.rect_pixels(ox, oy, rx, ry, W, H)
        v = place(rng, rec, triple, bits, channels, wpx * hpx, **plan)
        for f in range(3):
            if bits[f]:
                payload += S.pack_field(v[f], bits[f])
        classes.append(cls)
    data = S.assemble(B.VERSION, W, H, channels, 100, 1 | B.FLAG_MERGED, table, payload, rectangles=len(rects))
    return Stream(name, 2, channels, W, H, data, classes)


# ---- the corpus ----
# 27 x 27 blocks = 729 = 9^3: 12 units of 64, the last of 25 blocks whose last group holds one; 27 % 8 != 0, so groups straddle block rows
V1 = (("v1-rgba-216x216", 216, 216, 4, 11, True), ("v1-rgba-213x211", 213, 211, 4, 12, False), ("v1-rgba-212x216", 212, 216, 4, 13, False),
      ("v1-rgb-216x216", 216, 216, 3, 14, True), ("v1-rgb-213x211", 213, 211, 3, 15, False), ("v1-rgb-212x216", 212, 216, 3, 16, False))
V2 = (("v2-rgba-216x216", 216, 216, 4, 21), ("v2-rgba-213x211", 213, 211, 4, 22), ("v2-rgba-212x216", 212, 216, 4, 23), ("v2-rgb-213x211", 213, 211, 3, 24),
      ("v2-rgb-216x216", 216, 216, 3, 25))
_CORPUS = {}


def corpus(version):
    """the streams of one version, built once per process and never changed"""
    if version not in _CORPUS:
        decks = Decks(np.random.default_rng(1000 + version), rectangles=version == 2)
        if version == 1:
            _CORPUS[1] = [build_v1(name, W, H, ch, seed, decks, specials) for name, W, H, ch, seed, specials in V1]
        else:
            _CORPUS[2] = [build_v2(name, W, H, ch, seed, decks) for name, W, H, ch, seed in V2]
    return _CORPUS[version]


def decoded(stream, oracle):
    """the oracle's decode of a stream: computed once, shared, never changed"""
    if getattr(stream, "_decoded", None) is None:
        stream._decoded = stream.decode(oracle)
    return stream._decoded


# ---- the census ----
def entries(stream):
    """per block / rectangle of a stream, in table order: (entry, x0, y0, wpx, hpx, field values (3, hpx, wpx) of the pixels inside the image)"""
    if stream.blocked:
        hdr, table, payload = B.parse(stream.bytes)
    else:
        hdr, table, payload = S.parse(stream.bytes)
    bx = int(hdr["blocksX"])
    for g, e in enumerate(table):
        _, _, bits, o = S.entry_fields(e)
        if stream.blocked:
            x0, y0, wpx, hpx = B.rect_pixels(e["ox"], e["oy"], e["rx"], e["ry"], stream.W, stream.H)
            v = np.stack([f.reshape(hpx, wpx) for f in S.unpack_fields(payload, o, bits, wpx * hpx)])
        else:
            x0, y0 = 8 * (g % bx), 8 * (g // bx)
            wpx, hpx = min(8, stream.W - x0), min(8, stream.H - y0)
            v = np.stack([f.reshape(8, 8)[:hpx, :wpx] for f in S.unpack_fields(payload, o, bits, 64)])
        yield e, x0, y0, wpx, hpx, v.astype(np.int64)


def canonical(stream):
    """the layout rule: payloadWord is the exclusive prefix of the entries' words in table order, the payload has no other word, shifts stay in 0 .. 8 and the raw bits
    are what field_bits gives"""
    if stream.blocked:
        hdr, table, payload = B.parse(stream.bytes)
    else:
        hdr, table, payload = S.parse(stream.bytes)
    bx = int(hdr["blocksX"])
    at = 0
    for g, e in enumerate(table):
        _, shift, bits, o = S.entry_fields(e)
        want_bits, raw = S.field_bits(shift, e, stream.channels)
        if max(shift) > 8 or o != 8 * at or bits != want_bits or int(e["shift"]) >> 24 != raw:
            return False
        if stream.blocked:
            _, _, wpx, hpx = B.rect_pixels(e["ox"], e["oy"], e["rx"], e["ry"], stream.W, stream.H)
            at += sum(S.field_words(wpx * hpx, b) for b in bits)
        else:
            at += sum(bits)
    return at == int(hdr["payloadWords"]) and 8 * at == len(payload) and bx <= 64 and int(hdr["blocksY"]) <= 64


def census(streams, oracle):
    """What a list of streams of ONE version reaches, from their bytes alone -> a dict of plain counts (the golden JSON keeps it).  The conditions C1 .. C8 of
    check_census() are statements about this dict."""
    version = streams[0].version
    triples = {3: set(), 4: set()}
    escapes, fields, groups, geometry, shapes = set(), set(), set(), set(), set()
    odd_bits, ragged_bits = set(), set()
    wrapped = 0
    inside = {c: np.zeros((4, 2), dtype=np.int64) for c in CLASSES}
    below, above = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    class_count = dict.fromkeys(CLASSES, 0)
    over_positions = set()
    lane3_large = 0
    rect_counts = []
    for st in streams:
        assert st.version == version and canonical(st), st.name
        want = decoded(st, oracle)
        ch = st.channels
        geometry.add("whole" if st.W % 8 == 0 and st.H % 8 == 0 else "ragged" if st.W % 8 and st.H % 8 and st.W % 4 else "x%8==4" if st.W % 8 == 4 else "other")
        large_of, alpha_of = [], []
        for k, (e, x0, y0, wpx, hpx, v) in enumerate(entries(st)):
            rec, (_, shift, bits, _) = rec_array(e), S.entry_fields(e)
            sw = int(e["shift"])
            cls = classify(rec)
            assert cls == st.classes[k], (st.name, k, cls, st.classes[k])
            class_count[cls] += 1
            triples[ch].add(tuple(shift))
            if ch == 4:
                escapes.add((tuple(shift), sw >> 24))
            else:
                lane3_large += int(np.abs(rec[:, 3]).max() > LIMIT)
            if cls == "over":
                p = int(np.argmax(np.abs(rec).reshape(-1)))
                over_positions.add((ch, p, int(np.sign(rec.reshape(-1)[p]))))
            whole = (wpx * hpx) % 64 == 0
            for f in range(3):
                b = bits[f]
                if b and whole:
                    fields.add((f, b, "zero" if not v[f].any() else "max" if (v[f] == (1 << b) - 1).all() else "other"))
                if b and version == 2:
                    if (wpx * hpx * b) % 64:
                        odd_bits.add(b)
                    if wpx % 8:
                        ragged_bits.add(b)
            n, _ = constants(rec, shift, ch)
            for f in range(3):  # C6: an escaped factor at 255 under an alpha normal of +-65535: the 32-bit product wraps
                if (sw >> (24 + f)) & 1 and abs(int(n[f, 3])) == 65535:
                    wrapped += int((v[f] == 255).sum())
            est = estimate(rec, shift, ch, v)
            got = np.clip(est, 0, 255)
            pix = (got[0] | (got[1] << 8) | (got[2] << 16) | (got[3] << 24)).astype(np.uint32)
            assert np.array_equal(pix, want[y0:y0 + hpx, x0:x0 + wpx]), (st.name, k, "the census's arithmetic is not the oracle's")
            for c in range(ch):
                inside[cls][c, 0] += int(((got[c] >= 1) & (got[c] <= 254)).sum())
                inside[cls][c, 1] += got[c].size
                below[c] += int((est[c] < 0).sum())
                above[c] += int((est[c] > 255).sum())
            large_of.append(is_large(rec))
            alpha_of.append(ch == 4 and any(rec[2 * f, 3] != rec[2 * f + 1, 3] for f in range(3)))
            if version == 2:
                rx, ry = int(e["rx"]), int(e["ry"])
                gx, gy = (st.W + 7) // 8, (st.H + 7) // 8
                if rx == 1 and ry == 1:
                    shapes.add("1x1")
                if ry == 1 and rx == gx:
                    shapes.add("full row strip")
                if rx == 1 and ry >= gy - 1:
                    shapes.add("full column strip")
                if ry == 1 and 1 < rx < gx:
                    shapes.add("k x 1")
                if rx == 1 and 1 < ry < gy - 1:
                    shapes.add("1 x k")
                if rx * ry > 64:
                    shapes.add("more than 64 blocks")
                if rx > 1 and ry > 1 and st.W % 8 and int(e["ox"]) + rx == gx:
                    shapes.add("clipped right edge")
                if rx > 1 and ry > 1 and st.H % 8 and int(e["oy"]) + ry == gy:
                    shapes.add("clipped bottom edge")
        if version == 2:
            rect_counts.append(len(large_of))
            table = B.parse(st.bytes)[1]
            order = np.lexsort((table["ox"], table["oy"]))
            if not np.array_equal(order, np.arange(len(table))):
                shapes.add("shuffled")
        else:
            nb = len(large_of)
            bx = (st.W + 7) // 8
            if bx % 8:
                groups.add("groups straddle block rows")
            if nb % 64:
                groups.add("short last unit")
                if (nb % 64) % 8:
                    groups.add("short last group")
            for unit in range(0, nb, 64):
                for g0 in range(unit, min(unit + 64, nb), 8):
                    lg = large_of[g0:min(g0 + 8, unit + 64, nb)]
                    if len(lg) < 8:
                        continue
                    kind = "none" if not any(lg) else "all" if all(lg) else "one@%d" % lg.index(True) if sum(lg) == 1 else None
                    if kind:
                        groups.add((ch, bool(any(alpha_of[g0:g0 + 8])), kind))
    out = {
        "streams": len(streams),
        "entries": int(sum(class_count.values())),
        "classes": class_count,
        "triples_rgb": len(triples[3]),
        "triples_rgba": len(triples[4]),
        "triples_any": len(triples[3] | triples[4]),
        "escape_patterns_rgba": len(escapes),
        "field_kinds": len(fields),
        "field_kinds_missing": sorted("%d/%d/%s" % (f, b, k) for f in range(3) for b in range(1, 9) for k in ("zero", "max", "other") if (f, b, k) not in fields),
        "over_positions": len(over_positions),
        "rgb_records_with_large_lane3": lane3_large,
        "geometry": sorted(geometry),
        "wrapped_alpha_products": wrapped,
        "inside_1_254": {c: [round(float(inside[c][k, 0]) / max(1, int(inside[c][k, 1])), 4) for k in range(4)] for c in CLASSES},
        "true_clamps_below": [int(x) for x in below],
        "true_clamps_above": [int(x) for x in above],
    }
    if version == 1:
        out["group_kinds"] = sorted("%s/%s/%s" % (("rgba" if ch == 4 else "rgb"), ("alpha" if a else "flat"), k) for ch, a, k in (g for g in groups if isinstance(g, tuple)))
        out["group_layout"] = sorted(g for g in groups if isinstance(g, str))
    else:
        out["rectangles"] = rect_counts
        out["shapes"] = sorted(shapes)
        out["bits_with_partial_last_word"] = sorted(odd_bits)
        out["bits_on_ragged_width"] = sorted(ragged_bits)
    return out


def check_census(c, version):
    """C1 .. C8 (the issue's coverage conditions) as assertions about a census dict"""
    assert c["triples_any"] == 729, "C1 / C8: every shift triple"
    assert all(c["classes"][k] > 0 for k in CLASSES) and c["classes"]["wild"] * 10 < c["entries"], "the record classes, wild ones few"
    assert c["rgb_records_with_large_lane3"] > 0
    assert c["wrapped_alpha_products"] > 0, "C6: an alpha product beyond 2^31"
    for cls in ("fit", "limit", "over", "extreme"):
        assert min(c["inside_1_254"][cls][:3]) >= 0.5, ("C7", cls, c["inside_1_254"][cls])
        assert c["inside_1_254"][cls][3] >= 0.5, ("C7, alpha", cls, c["inside_1_254"][cls])
    assert min(c["true_clamps_below"]) > 0 and min(c["true_clamps_above"]) > 0, "C7: every channel clamps both ways"
    assert {"whole", "ragged", "x%8==4"} <= set(c["geometry"]), "C5 / C8"
    if version == 1:
        assert c["triples_rgb"] == 729 and c["triples_rgba"] == 729, "C1: every shift triple, for 3 and for 4 channels"
        assert c["escape_patterns_rgba"] == 1000, "C2: every triple with every subset of its shift-8 factors escaped"
        assert c["field_kinds"] == 72 and not c["field_kinds_missing"], "C3"
        assert c["over_positions"] == 96, "over: each of the 24 positions, both signs, 3 and 4 channels"
        want = {"%s/%s/%s" % (ch, a, k) for ch, alphas in (("rgba", ("alpha", "flat")), ("rgb", ("flat",))) for a in alphas for k in GROUP_KINDS}
        assert want <= set(c["group_kinds"]), ("C4", sorted(want - set(c["group_kinds"])))
        assert c["group_layout"] == ["groups straddle block rows", "short last group", "short last unit"], "C4"
    else:
        assert min(c["rectangles"]) > 64
        assert set(c["shapes"]) == {"1x1", "1 x k", "k x 1", "full row strip", "full column strip", "more than 64 blocks", "clipped right edge", "clipped bottom edge", "shuffled"}, "C8"
        assert c["bits_with_partial_last_word"] == list(range(1, 9)) and c["bits_on_ragged_width"] == list(range(1, 9)), "C8"


def group_kind(stream, g):
    """of block g of a version 1 stream: how k_stream_decode sees its group of 8 -- 'packed' or 'generic (n large of m)', and whether an alpha lane varies in it"""
    table = S.parse(stream.bytes)[1]
    unit = g // 64 * 64
    g0 = unit + (g - unit) // 8 * 8
    idx = range(g0, min(g0 + 8, unit + 64, len(table)))
    recs = [rec_array(table[i]) for i in idx]
    n = sum(is_large(r) for r in recs)
    alpha = stream.channels == 4 and any(r[2 * f, 3] != r[2 * f + 1, 3] for r in recs for f in range(3))
    return "%s, %s" % ("generic (%d large of %d)" % (n, len(recs)) if n else "packed", "alpha varies" if alpha else "alpha flat")


def describe_mismatch(stream, want, got, limit=4):
    """the first differing blocks / rectangles of a decode, with their class, shift word and (version 1) group kind"""
    out = []
    for k, (e, x0, y0, wpx, hpx, _) in enumerate(entries(stream)):
        if not np.array_equal(want[y0:y0 + hpx, x0:x0 + wpx], got[y0:y0 + hpx, x0:x0 + wpx]):
            yy, xx = np.argwhere(want[y0:y0 + hpx, x0:x0 + wpx] != got[y0:y0 + hpx, x0:x0 + wpx])[0]
            out.append("%s %d at (%d, %d): class %s, shift word 0x%08x%s; pixel (%d, %d) wants %08x, got %08x" % (
                "rectangle" if stream.blocked else "block", k, x0, y0, stream.classes[k], int(e["shift"]), "" if stream.blocked else ", group " + group_kind(stream, k),
                x0 + xx, y0 + yy, int(want[y0 + yy, x0 + xx]), int(got[y0 + yy, x0 + xx])))
            if len(out) == limit:
                break
    return "%s: %s" % (stream.name, "; ".join(out))
