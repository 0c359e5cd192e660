"""Range edges: every packed kernel at the LAST shape its range check admits, and the routing one base further.

The packed kernels keep score << ts in 16 bits (ts = 4: "x16", ts = 2: "x4"; -32768 is -inf).  packed_ok (at_hip.hip) alone keeps a
batch inside that range: a shape is admitted iff scale * (lo + hi + slack) < 32768, and the kernels get thresh16 = -32768 +
scale * (hi + slack).  The other parity tests use fixed shapes that stay at 40 .. 60 % of the range; here every case is the last
admitted shape of a family of shapes, with inputs that store exactly scale * hi (everything matches) next to the deepest cells the
mode has (nothing matches, one-sided gaps) -- in the two halves of one 32-bit word.

Three parts:
  1. admits / edge: packed_ok restated, the last admitted shape along a family, the case table and its inputs;
  2. cells: a plain DP by anti-diagonals (numpy int64) that returns the smallest and the largest finite cell of all matrices, and
     the conditions on the inputs (unmarked tests: no GPU);
  3. GPU parity: the flip of the routing at the edge, every kernel family at its edge, the other range gates as admitted / refused
     pairs -- every pair and every field against the oracle.

    python3 tests/test_range_edges.py        # prints, per case, the edge shape, thresh16, reach_hi and reach_lo (no GPU)
"""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle as O

# =============================================================================================== 1. the restated bound


def admits(mode, scoring, l1, l2, ts, use_jump=False):
    """(admitted, thresh16): packed_ok of aligntools/c_amd/csrc/at_hip.hip restated -- overlap :633-642, the affine modes :643-660.
    scoring = (m, u, o, e[, j]).  A change there needs one here."""
    m, u, o, e = scoring[:4]
    j = scoring[4] if len(scoring) > 4 else -10
    scale = 1 << ts
    if l1 < 1 or l2 < 1:                                                        # :632
        return False, 0
    if mode == "overlap":
        if ts != 2 or m < 0 or u > 0 or o > 0:                                  # :636
            return False, 0
        lo = abs(o) * max(l1, l2) + abs(u) + 16                                 # :637
        hi, slack = m * min(l1, l2), abs(o) + abs(u) + 3                        # :638
    else:
        if mode not in ("global", "local", "fit") or m < 0 or u > 0 or o > 0 or e > 0:   # :643-644
            return False, 0
        hasj = mode == "fit" and use_jump                                       # :645
        if hasj and (j > 0 or abs(j - o) * scale > 32000):                      # :646
            return False, 0
        lo = 3 * abs(o) + (abs(j) if hasj else 0) + abs(u) * min(l1, l2) + abs(e) * max(l1, l2) + 16   # :651-652
        if mode == "local":
            lo = abs(o) + abs(u) + abs(e) + 16                                  # :655
        hi, slack = m * min(l1, l2), abs(o) + abs(e) + 3                        # :656-657
    if scale * (lo + hi + slack) >= 32768:                                      # :639, :658
        return False, 0
    return True, -32768 + scale * (hi + slack)                                  # :640, :659


FAMILIES = {
    "square": lambda l: (l, l),
    "long1": lambda l: (l, 16),          # global only (fit needs l1 <= l2)
    "long2": lambda l: (16, l),
    "long2w": lambda l: (40, l),
}


def edge(mode, scoring, ts, shape, use_jump=False, top=1 << 16):
    """the last l at which the family's shape is admitted (the bound grows with either length), or 0"""
    f = FAMILIES[shape]
    if not admits(mode, scoring, *f(1), ts, use_jump)[0]:
        return 0
    lo, hi = 1, top
    while lo < hi:                                                              # admits(lo) holds; the first refusal lies in (lo, hi]
        mid = (lo + hi + 1) // 2
        if admits(mode, scoring, *f(mid), ts, use_jump)[0]:
            lo = mid
        else:
            hi = mid - 1
    return lo


# ----------------------------------------------------------------------------------------------- the cases

# row classes of the packed kernels (at_classes.h): the group width a uniform batch of l1-base reads runs on with scores x16
CLASS_TOPS = ((76, 4), (152, 8), (304, 16), (608, 32), (1024, 64))
ONE_STRIP_TOP = {"local": 608, "global": 512, "fit": 416, "fitj": 416}    # the longest read on the 32-lane groups (kTopLocal ..)
GROUPS = {4: "16x4-lane groups", 8: "8x8-lane groups", 16: "4x16-lane groups", 32: "2x32-lane groups", 64: "1x64-lane groups"}


def group_of(kind, l1, ts):
    """lanes per group of a uniform batch (layout16_for, at_hip.hip :573-597): scores x4 and overlap run on the 64-lane group"""
    if ts != 4 or kind == "overlap":
        return 64
    for top, g in CLASS_TOPS[:3]:
        if l1 <= top:
            return g
    return 32 if l1 <= ONE_STRIP_TOP[kind] else 64


def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


class Case:
    """kind: global / local / fit / fitj (fit -s) / overlap; the shape is the last one of its family that packed_ok admits with ts"""

    def __init__(self, kind, sc, ts, family="square"):
        self.kind, self.sc, self.ts, self.family = kind, tuple(sc), ts, family
        self.mode = "fit" if kind == "fitj" else kind
        self.uj = kind == "fitj"
        self.scale = 1 << ts
        self.l = edge(self.mode, self.sc, ts, family, self.uj)
        assert 16 < self.l <= 1400, (kind, sc, ts, family, self.l)
        self.l1, self.l2 = FAMILIES[family](self.l)
        self.thresh16 = admits(self.mode, self.sc, self.l1, self.l2, ts, self.uj)[1]
        self.hi = self.sc[0] * min(self.l1, self.l2)
        self.g = group_of(kind, self.l1, ts)
        self.bits = 2 if _fits_byte(kind, self.sc) else 8
        self.id = "%s-x%d-%s-m%du%do%de%d%s" % (kind, self.scale, family, self.sc[0], -self.sc[1], -self.sc[2], -self.sc[3],
                                                "j%d" % -self.sc[4] if self.uj else "")
        self._pairs = {}

    def shape(self, step=0):
        return FAMILIES[self.family](self.l + step)

    def sites(self, step=0):
        l2 = self.shape(step)[1]
        return [l2 // 3, l2 // 2, l2 // 2 + 1] if self.uj else []

    def engine(self, step=0):
        """what last_config must name at the edge (0) and one base further (1)"""
        ts = self.ts
        if step and not admits(self.mode, self.sc, *self.shape(step), ts, self.uj)[0]:
            ts = 2 if ts == 4 and admits(self.mode, self.sc, *self.shape(step), 2, self.uj)[0] else 0
        return "packed16 x%d " % (1 << ts) if ts else "int32"

    def two_pass(self):
        """has the edge shape CK kernels (at_k16_tp.hip, at_k16_tp64.hip: 8 lanes x 19 rows with scores x16, 64 lanes x 16 rows)?"""
        if self.kind == "overlap":
            return False
        if self.ts == 4:
            return 129 <= self.l1 <= 152 or max(512, ONE_STRIP_TOP[self.kind]) < self.l1 <= 1024
        return self.kind != "fitj" and 512 < self.l1 <= 1024

    def pairs(self, step=0):
        """the unique pairs of the case at its edge (step 0) or one base further along the family (step 1), in batch order: an all-match
        and a nothing-matches alignment share a 32-bit word in both orders (alignments 2 k and 2 k + 1 are the halves of one word)"""
        if step not in self._pairs:
            l1, l2 = self.shape(step)
            self._pairs[step] = fixed_pairs(l1, l2, self.mode) + related_pairs(l1, l2, 4, _seed(self.id) + step)
            assert all((len(a), len(b)) == (l1, l2) for a, b in self._pairs[step]), self.id
        return self._pairs[step]


def _seed(text):
    import zlib
    return zlib.crc32(text.encode())


def _fits_byte(kind, sc):
    """scores_fit_byte (at_hip.hip :523-532): the host entries pack 2-bit words iff the scaled scores fit the signed-byte LUT"""
    m, u, o = sc[:3]
    if kind == "overlap":
        return all(abs(v) <= 127 for v in (16 * (m - o), 16 * (u - o), m - 2 * o, u - 2 * o))
    return abs(16 * m) <= 127 and abs(16 * u) <= 127


def fixed_pairs(l1, l2, mode="global"):
    """the six fixed pairs of a shape (eight alignments: the first two twice)"""
    rng = random.Random(l1 * 100003 + l2)
    lo, hi = min(l1, l2), max(l1, l2)
    R = _rnd(rng, hi + hi // 4 + 8, "ACG")                   # (no T: a run of T matches nothing of R)
    match = (R[:l1], R[:l2])                                 # every diagonal cell a match: the largest cell is exactly m * min(l1, l2)
    nomatch = ("A" * l1, "C" * l2)
    d = hi - lo if hi > lo else hi // 4                      # a one-sided gap of the whole length difference (square: a quarter)
    if l1 == l2:
        gap = (R[:l1], R[d:l1] + "T" * d)
        mid = (R[:l1 // 2] + R[l1 // 2 + d:l1 + d], R[:l2])  # all-match around one gap of d in the middle
    elif l1 > l2:
        gap = (R[:l1], R[d:l1])
        mid = (R[:l1], R[:l2 // 2] + R[l2 // 2 + d:l1])
    else:
        gap = (R[d:l2], R[:l2])
        mid = (R[:l1 // 2] + R[l1 // 2 + d:l2], R[:l2])
    periodic = (("AAC" * l1)[:l1], ("AC" * l2)[:l2])         # ties all over
    h1, h2 = l1 // 2, l2 // 2
    halves = (R[:h1] + "A" * (l1 - h1), R[:h2] + "T" * (l2 - h2))
    return [match, nomatch, nomatch, match, gap, mid, periodic, halves]


def related_pairs(l1, l2, n, seed):
    """s2 from s1 by scattered edits, cut or filled to l2 bases"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        a = _rnd(rng, l1)
        t = list(a)
        for _ in range(1 + l1 // 12):
            q = rng.randrange(len(t))
            r = rng.random()
            if r < 0.5:
                t[q] = rng.choice("ACGT")
            elif r < 0.75 and len(t) > 1:
                del t[q]
            else:
                t.insert(q, rng.choice("ACGT"))
        out.append((a, (_rnd(rng, rng.randint(0, max(0, l2 - l1))) + "".join(t) + _rnd(rng, l2))[:l2]))
    return out


# Scorings chosen so that the x16 edge of each mode falls into every row class (reads of up to 76, 152, 304, 608 and 1 024 bases: the
# 4-, 8-, 16-, 32- and 64-lane groups), with 2-bit words (m <= 7: the LUT forms, for local the profile forms) and with byte words
# (m >= 8), and the x4 edge on the 64-lane group with 4 rows per lane (strips) and with 16.
X16 = {
    "local": [(27, -1, -1, -1), (15, -8, -6, -2), (14, -1, -1, -1), (8, -8, -9, -2), (7, -7, -9, -2), (5, -4, -10, -1), (3, -1, -1, -3),
              (2, -1, -1, -1)],
    "global": [(30, -20, -10, -5), (7, -7, -9, -2), (6, -5, -10, -2), (8, -4, -3, -2), (5, -4, -10, -1), (3, -1, -1, -3), (1, -3, -4, -1),
               (1, -1, -4, -1)],
    "fit": [(30, -20, -10, -5), (6, -5, -10, -2), (8, -4, -3, -2), (3, -1, -1, -3), (1, -3, -4, -1), (1, -1, -4, -1)],
    "fitj": [(6, -5, -9, -2, -12), (1, -1, -4, -1, -6)],
}
X4 = {
    "local": [(7, -7, -9, -2), (8, -8, -9, -2), (16, -4, -4, -4)],
    "global": [(3, -3, -5, -2), (3, -1, -1, -3), (7, -7, -9, -2)],
    "fit": [(3, -3, -5, -2), (9, -9, -12, -3)],
    "fitj": [(3, -3, -5, -2, -9)],
    "overlap": [(40, -9, -20, -3), (7, -7, -9, -2), (3, -3, -5, -2), (1, -2, -5, -1), (2, -2, -5, -2)],
}
SKEWED = [("global", (7, -7, -9, -2), "long2"), ("fit", (7, -7, -9, -2), "long2"), ("global", (10, -10, -10, -10), "long1"), ("global", (30, -20, -10, -5), "long1"), ("global", (9, -9, -12, -3), "long1"),
          ("global", (10, -10, -10, -10), "long2"), ("global", (16, -4, -4, -4), "long2w"),
          ("fit", (10, -10, -10, -10), "long2"), ("fit", (16, -4, -4, -4), "long2w")]


def _cases():
    out = [Case(kind, sc, 4) for kind, scs in X16.items() for sc in scs]
    out += [Case(kind, sc, 4, fam) for kind, sc, fam in SKEWED]
    out += [Case(kind, sc, 2) for kind, scs in X4.items() for sc in scs]
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# =============================================================================================== 2. the cells of the matrices

NEG = -(1 << 40)


def cells(kind, sc, pairs, sites=()):
    """Plain DP by anti-diagonals over the pairs of ONE shape, numpy int64, three states (M, L, U; J for fit -s; overlap: M alone)
    as oracle/at_oracle.c fills them: dict(score = the score of every pair, lo / hi = the smallest and the largest finite cell of
    all matrices of every pair, borders included)."""
    m, u, o, e = sc[:4]
    g = sc[4] if len(sc) > 4 else -10
    a = np.array([np.frombuffer(p[0].encode(), dtype=np.uint8) for p in pairs])
    b = np.array([np.frombuffer(p[1].encode(), dtype=np.uint8) for p in pairs])
    P, l1, l2 = len(pairs), a.shape[1], b.shape[1]
    names = ("M",) if kind == "overlap" else ("M", "L", "U", "J") if kind == "fitj" else ("M", "L", "U")
    listed = np.zeros(l2 + 1, dtype=bool)
    listed[[s for s in sites if 0 <= s <= l2]] = True

    def border(i, j):
        if kind == "global":
            return dict(M=0 if i == j == 0 else NEG, L=o + e * i if j == 0 else NEG, U=o + e * j if i == 0 else NEG)
        if kind == "local":
            return dict(M=0, L=0, U=0)
        if kind == "overlap":
            return dict(M=0 if j == 0 else NEG)
        return dict(M=0 if i == 0 else NEG, U=0 if i == 0 else NEG, L=NEG, J=NEG)    # fit: row 0 is free, column 0 closed

    def fresh():
        return {k: np.full((P, l1 + 1), NEG, dtype=np.int64) for k in names}

    d1, d2 = fresh(), fresh()                                 # the diagonals d - 1 and d - 2, indexed by the row
    lo = np.full(P, -NEG, dtype=np.int64)
    hi = np.full(P, NEG, dtype=np.int64)
    score = np.full(P, NEG, dtype=np.int64)
    for d in range(l1 + l2 + 1):
        cur = fresh()
        ilo, ihi = max(1, d - l2), min(l1, d - 1)
        if ilo <= ihi:
            i = np.arange(ilo, ihi + 1)
            s = np.where(a[:, i - 1] == b[:, d - i - 1], m, u)
            if kind == "overlap":
                cur["M"][:, i] = np.maximum(np.maximum(d1["M"][:, i] + o, d2["M"][:, i - 1] + s), d1["M"][:, i - 1] + o)
            else:
                best = np.maximum(np.maximum(d2["L"][:, i - 1], d2["M"][:, i - 1]), d2["U"][:, i - 1])
                if kind == "fitj":
                    best = np.maximum(best, d2["J"][:, i - 1])
                cur["M"][:, i] = np.maximum(best + s, 0) if kind == "local" else best + s
                cur["L"][:, i] = np.maximum(d1["L"][:, i - 1] + e, d1["M"][:, i - 1] + o)
                cur["U"][:, i] = np.maximum(d1["M"][:, i] + o, d1["U"][:, i] + e)
                if kind == "fitj":                            # the M -> J opening exactly where column j - 1 is NOT listed
                    cur["J"][:, i] = np.maximum(np.where(listed[d - i - 1], NEG, d1["M"][:, i] + g), d1["J"][:, i])
            for k in names:
                cur[k][cur[k] < NEG // 2] = NEG
        if d <= l2:
            for k in names:
                cur[k][:, 0] = border(0, d)[k]
        if d <= l1:
            for k in names:
                cur[k][:, d] = border(d, 0)[k]
        for k in names:
            x = cur[k]
            fin = x > NEG // 2
            lo = np.minimum(lo, np.where(fin, x, -NEG).min(axis=1))
            hi = np.maximum(hi, np.where(fin, x, NEG).max(axis=1))
        j = d - l1                                            # the cell of the last row on this diagonal
        if kind == "local":
            score = np.maximum(score, cur["M"][:, 1:].max(axis=1) if d >= 2 else score)
        elif kind == "global":
            if d == l1 + l2:
                score = np.maximum(np.maximum(cur["L"][:, l1], cur["M"][:, l1]), cur["U"][:, l1])
        elif 0 <= j < l2:                                     # fit, overlap: the end cell over the columns 0 .. l2 - 1 of the last row
            score = np.maximum(score, cur["M"][:, l1])
            if kind != "overlap":
                score = np.maximum(score, cur["L"][:, l1])
        d2, d1 = d1, cur
    return dict(score=score, lo=lo, hi=hi)


_REACH = {}


def reach(case):
    """(reach_hi, reach_lo, per-pair cells): scale * the largest cell, and how far scale * the smallest cell lies above thresh16"""
    if case.id not in _REACH:
        c = cells(case.kind, case.sc, case.pairs(), case.sites())
        _REACH[case.id] = (case.scale * int(c["hi"].max()), case.scale * int(c["lo"].min()) - case.thresh16, c)
    return _REACH[case.id]


_ORACLE = {}


def _oracle(mode, sc, uj, sites, pairs):
    """the oracle's result for every distinct pair, once per scoring, site list and pair"""
    from concurrent.futures import ThreadPoolExecutor
    memo = _ORACLE.setdefault((mode, tuple(sc), uj, tuple(sites)), {})
    todo = [p for p in dict.fromkeys(pairs) if p not in memo]
    if todo:
        O.align(O.LOCAL, "A", "AA")                  # (loads the library before the threads start)
        full = tuple(sc) + ((-10,) if len(sc) == 4 else ())
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            res = list(ex.map(lambda p: O.align(O.MODE_NAMES[mode], p[0], p[1], *full, uj, list(sites)), todo))
        memo.update(zip(todo, res))
    return [memo[p] for p in pairs]


def test_restated_bound_on_the_known_edges():
    """the last admitted square shapes as the issue's table states them"""
    want = {("local", (2, -2, -5, -2)): (1006, 4078), ("local", (7, -7, -9, -2)): (285, 1163), ("global", (7, -7, -9, -2)): (124, 508),
            ("fit", (7, -7, -9, -2)): (124, 508), ("global", (1, -1, -4, -1)): (670, 2718), ("overlap", (1, -2, -5, -1)): (0, 1360)}
    for (mode, sc), w in want.items():
        assert (edge(mode, sc, 4, "square"), edge(mode, sc, 2, "square")) == w, (mode, sc)


def test_dp_matches_the_oracle():
    """cells() on 400 small random pairs, every mode: the oracle's scores"""
    rng = random.Random(0xCE11)
    for k in range(400):
        kind = ("global", "local", "fit", "fitj", "overlap")[k % 5]
        l1 = rng.randint(1, 24)
        l2 = rng.randint(l1 if kind in ("fit", "fitj") else 1, 30)
        sc = (rng.randint(0, 9), -rng.randint(0, 9), -rng.randint(0, 12), -rng.randint(0, 4)) + ((-rng.randint(0, 15),) if kind == "fitj" else ())
        sites = sorted(rng.sample(range(l2 + 1), min(3, l2))) if kind == "fitj" else []
        alpha = "AC" if k % 3 == 0 else "ACGT"
        p = (_rnd(rng, l1, alpha), _rnd(rng, l2, alpha))
        r = _oracle("fit" if kind == "fitj" else kind, sc, kind == "fitj", sites, [p])[0]
        c = cells(kind, sc, [p], sites)
        assert r["rc"] == 0 and int(c["score"][0]) == r["score"], (kind, sc, sites, p, int(c["score"][0]), r["score"])
        assert int(c["lo"][0]) <= r["score"] <= int(c["hi"][0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_is_the_last_admitted_shape(case):
    assert admits(case.mode, case.sc, *case.shape(0), case.ts, case.uj)[0]
    assert not admits(case.mode, case.sc, *case.shape(1), case.ts, case.uj)[0]
    assert max(case.shape(1)) <= 1400
    if case.ts == 2:                                          # the x4 cases are x4 cases: scores x16 do not admit them
        assert not admits(case.mode, case.sc, *case.shape(0), 4, case.uj)[0]
    else:                                                     # one base further the scores x4 take over
        assert case.engine(1) == "packed16 x4 "


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_inputs_reach_the_edges_of_the_range(case):
    """caps, not measurements: the all-match pair stores exactly scale * hi where the mode lets a path start anywhere; the x16
    local cases lie in the sign-bit half of an unsigned 16-bit word; the skewed global cases come within scale * (|u| min(l1, l2) +
    3 |o| + 32) of thresh16; and nothing leaves the range the bound promises"""
    reach_hi, reach_lo, c = reach(case)
    m, u, o, e = case.sc[:4]
    assert reach_hi <= case.scale * case.hi and reach_lo > 0, (case.id, reach_hi, reach_lo)
    assert case.scale * int(c["lo"].min()) > -32768 and reach_hi < 32768
    if case.kind in ("local", "overlap"):
        for k in (0, 3):
            assert case.scale * int(c["hi"][k]) == case.scale * case.hi, (case.id, k)
    if case.kind == "local" and case.ts == 4:
        assert reach_hi >= 1 << 14, (case.id, reach_hi)
    if case.kind == "global" and case.family != "square":
        assert reach_lo < case.scale * (abs(u) * min(case.l1, case.l2) + 3 * abs(o) + 32), (case.id, reach_lo)


def test_the_table_covers_every_class():
    """x16: every mode's edges in every row class, 2-bit and byte words in each mode; one local case stores at least 31 000; x4: the
    64-lane group with one strip of 16 rows per lane (513 .. 1 024 bases) and with strips of 4; overlap with 4 and 16 rows per lane"""
    for kind in ("local", "global", "fit"):
        seen = {c.g for c in CASES if c.kind == kind and c.ts == 4}
        assert seen == {4, 8, 16, 32, 64}, (kind, seen)
        assert {c.bits for c in CASES if c.kind == kind and c.ts == 4} == {2, 8}, kind
    assert {c.g for c in CASES if c.kind == "fitj" and c.ts == 4} == {8, 64}
    assert max(reach(c)[0] for c in CASES if c.kind == "local" and c.ts == 4) >= 31000
    for kind in ("local", "global", "fit"):
        l1s = [c.l1 for c in CASES if c.kind == kind and c.ts == 2]
        assert any(512 < l <= 1024 for l in l1s) and any(l <= 512 or l > 1024 for l in l1s), (kind, l1s)
    ovl = [c.l1 for c in CASES if c.kind == "overlap"]
    assert any(l <= 256 for l in ovl) and any(256 < l <= 1024 for l in ovl) and any(l > 1024 for l in ovl), ovl
    assert any(c.two_pass() and c.g == 8 for c in CASES) and any(c.two_pass() and c.ts == 2 for c in CASES)


def test_baseline_shapes_keep_their_engines_under_the_restated_bound():
    """C2 and C4 with scores x16, C3 and C5 with scores x4 (bench.py, WORKLOADS): a tightened bound must not move them"""
    assert admits("local", (2, -2, -5, -2), 150, 150, 4)[0]
    assert not admits("global", (1, -1, -4, -1), 1024, 1024, 4)[0] and admits("global", (1, -1, -4, -1), 1024, 1024, 2)[0]
    assert admits("fit", (2, -2, -5, -1, -10), 150, 500, 4, True)[0]
    assert admits("overlap", (1, -2, -5, -1), 1000, 1000, 2)[0]


# =============================================================================================== 3. GPU parity

KNOBS_CLEARED = ("AT_TWO_PASS", "AT_TP_SPLIT", "AT_GROUP", "AT_STORE", "AT_NO_PACKED", "AT_WS_CAP_MB", "AT_WALK_TEAMS", "AT_CK_PIECE_PAIRS",
                 "AT_TAIL_SPLIT", "AT_ROWS_PER_LANE", "AT_CK_CAP_MB", "AT_NO_PACKED_OVERLAP", "AT_RAGGED_PACKED", "AT_AUTO_UNIFORM")
ENGINES = {
    # name: (environment, what last_config must hold, what it must not hold)
    "onepass": ({"AT_TWO_PASS": "0"}, (), ("two-pass",)),
    "rounds": ({"AT_TWO_PASS": "2", "AT_TP_SPLIT": "0"}, ("two-pass",), ("walk kernel",)),
    "walk": ({"AT_TWO_PASS": "2", "AT_TP_SPLIT": "1", "AT_WALK_TEAMS": "0"}, ("walk kernel",), ("teams",)),
    "teams": ({"AT_TWO_PASS": "2", "AT_TP_SPLIT": "1", "AT_WALK_TEAMS": "1"}, ("walk kernel", "teams"), ()),
}
SEEN = []        # (test, case or gate, last_config) of every launch of this module: test_every_family_was_seen reads it


@pytest.fixture(scope="module")
def al():
    import aligntools.c_amd as A
    before = os.environ.get("AT_PACKED_MIN_ROUNDS")
    os.environ["AT_PACKED_MIN_ROUNDS"] = "0"   # small test batches must still reach the 64-lane packed kernels
    a = A.Aligner()
    yield a
    a.close()
    if before is None:
        os.environ.pop("AT_PACKED_MIN_ROUNDS", None)
    else:
        os.environ["AT_PACKED_MIN_ROUNDS"] = before


@pytest.fixture
def env(monkeypatch):
    """one chunk per host-entry call (a chunk on a helper handle would keep its own last_config), no knob from outside"""
    for name in KNOBS_CLEARED:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    monkeypatch.setenv("AT_PACKED_MIN_ROUNDS", "0")
    return monkeypatch


def batch_size(l1):
    """pairs of a batch: more than one wave of every group width, a dozen or two of the long shapes"""
    return 72 if l1 <= 304 else 24 if l1 <= 608 else 12


def check(al, mode, sc, uniq, n, tb, uj=False, sites=(), where=None):
    """the batch uniq[0], uniq[1], ... repeated to n pairs (n even: the halves of a word stay together) against the oracle on the
    unique pairs: score, end cell, state and, with tracebacks, nops and ops.  Returns last_config."""
    full = tuple(sc) + ((-10,) if len(sc) == 4 else ())
    refs = _oracle(mode, sc, uj, sites, uniq)
    assert all(r["rc"] == 0 for r in refs), where
    al.set_scoring(*full, uj, list(sites))
    pairs = [uniq[k % len(uniq)] for k in range(n)]
    res = al.align_batch(mode, pairs, traceback=tb, render=False)
    cfg = al.last_config
    SEEN.append((where, cfg))
    for k in range(n):
        r = refs[k % len(uniq)]
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]))
        assert got == (r["score"], r["end_i"], r["end_j"], r["state"]), (k, got, (r["score"], r["end_i"], r["end_j"], r["state"]), where, cfg)
        if tb:
            assert int(res["nops"][k]) == len(r["ops"]) and res["ops"][k] == r["ops"], (k, where, cfg)
    return cfg


def _even(pairs, n):
    return max(n, len(pairs)) + max(n, len(pairs)) % 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_routing_flips_at_the_edge(al, env, case):
    """the default route: the last admitted shape runs on the packed kernels with the case's scale, one base further along the family
    on the next engine (scores x4, or the int32 kernel) -- and both equal the oracle"""
    for step in (0, 1):
        uniq = case.pairs(step)
        l1 = case.shape(step)[0]
        cfg = check(al, case.mode, case.sc, uniq, _even(uniq, batch_size(l1)), True, case.uj, case.sites(step), ("flip", case.id, step))
        assert case.engine(step) in cfg, (case.id, step, cfg)
        assert "bits=%d" % case.bits in cfg, (case.id, step, cfg)
        if step == 0 and case.kind != "overlap":
            assert GROUPS[case.g] in cfg, (case.id, cfg)


def rows_x4(l1, what):
    """rows per lane on the 64-lane group with scores x4 (layout16_for, at_hip.hip :562-564): one strip of 1 024 rows once that is
    fewer instructions than strips of 256 -- the scores-only sweeps and packed overlap price a step differently"""
    a, b = ((16 * 9 + 45), (4 * 9 + 30)) if what == "overlap" else ((16 * 11 + 25), (4 * 11 + 25))
    return 16 if ((l1 + 1023) // 1024) * a < ((l1 + 255) // 256) * b else 4


def _engines(case):
    return ("onepass",) + (("rounds", "walk", "teams") if case.two_pass() else ())


@pytest.mark.gpu
@pytest.mark.parametrize("case,engine", [(c, e) for c in CASES for e in _engines(c)], ids=lambda v: v.id if isinstance(v, Case) else v)
def test_every_family_at_its_edge(al, env, case, engine):
    """the one-pass kernels with tracebacks and scores only (scores x4: strips of 4 rows per lane with tracebacks, one strip of 16
    without, past 512 bases); where the shape has CK kernels the rounds inside the sweep's kernel and the walk kernel with and without
    teams; overlap with 4 and with 16 rows per lane, and with the int32 kernel for the scores alone"""
    knobs, must, must_not = ENGINES[engine]
    for name, value in knobs.items():
        env.setenv(name, value)
    uniq = case.pairs()
    n = _even(uniq, batch_size(case.l1))
    for tb in (True, False) if engine == "onepass" else (True,):
        cfg = check(al, case.mode, case.sc, uniq, n, tb, case.uj, case.sites(), ("family", case.id, engine, tb))
        if case.kind == "overlap" and not tb:
            assert "int32" in cfg, (case.id, cfg)          # (the packed overlap kernel exists with pointers only)
            continue
        assert case.engine() in cfg and "bits=%d" % case.bits in cfg, (case.id, engine, tb, cfg)
        if tb or engine != "onepass":
            for text in must:
                assert text in cfg, (text, case.id, engine, cfg)
        for text in must_not:
            assert text not in cfg, (text, case.id, engine, cfg)
        if case.kind == "overlap":
            assert "rows/lane=%d " % rows_x4(case.l1, "overlap") in cfg, (case.id, cfg)
        elif case.ts == 2 and engine == "onepass":
            assert "rows/lane=%d " % (4 if tb else rows_x4(case.l1, "scores")) in cfg, (case.id, tb, cfg)
        elif engine != "onepass":
            assert "rows/lane=%d " % (19 if case.g == 8 else 16) in cfg, (case.id, engine, cfg)
    if case.kind == "overlap" and rows_x4(case.l1, "overlap") == 16:   # the other strip height, forced
        env.setenv("AT_ROWS_PER_LANE", "4")
        cfg = check(al, case.mode, case.sc, uniq, n, True, where=("family", case.id, "rows 4"))
        assert "packed16 x4 " in cfg and "rows/lane=4 " in cfg, (case.id, cfg)


def _cut(rng, uniq, l1, l2, lo1, lo2, n):
    """a ragged batch: the first two pairs keep the full shape, the others are prefixes of the unique pairs, no shorter than lo1 x lo2"""
    out = list(uniq[:2])
    while len(out) < n:
        a, b = uniq[len(out) % len(uniq)]
        c1 = rng.randint(lo1, l1)
        out.append((a[:c1], b[:rng.randint(max(lo2, c1), l2) if l2 >= l1 else rng.randint(lo2, l2)]))
    return out


RAGGED = [("global-x16-square-m7u7o9e2", 81, 8), ("fit-x16-square-m8u4o3e2", 81, 8), ("local-x16-square-m5u4o10e1", 305, 32),
          ("global-x16-square-m1u3o4e1", 305, 32), ("overlap-x4-square-m40u9o20e3", 60, 64), ("overlap-x4-square-m3u3o5e2", 600, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,lo1,g", RAGGED, ids=[r[0] for r in RAGGED])
def test_ragged_frames_at_the_edge(al, env, cid, lo1, g):
    """max_len1 x max_len2 is the last admitted shape, the lengths lie below it within one row class: frames on the 8- and the
    32-lane groups and ragged overlap; one base further the batch leaves the packed kernels (frames have no scores x4)"""
    case = BY_ID[cid]
    for step in (0, 1):
        l1, l2 = case.shape(step)
        rng = random.Random(_seed(cid) + step)
        pairs = _cut(rng, case.pairs(step), l1, l2, lo1, lo1, 80 if l1 <= 608 else 64)
        cfg = check(al, case.mode, case.sc, pairs, len(pairs), True, where=("ragged", cid, step))
        if step == 0:
            assert case.engine() in cfg and "ragged frames" in cfg and GROUPS[g] in cfg, (cid, cfg)
        else:
            assert "int32" in cfg and "packed16" not in cfg, (cid, cfg)


# ----------------------------------------------------------------------------------------------- the other gates

def _shape_pairs(l1, l2, seed, n=4):
    return fixed_pairs(l1, l2) + related_pairs(l1, l2, n, seed)


@pytest.mark.gpu
def test_gate_jump_opening_within_32000(al, env):
    """fit -s: |j - o| * scale <= 32000 (at_hip.hip :646).  1/0/0/0 with j = -8000 is admitted with scores x4 up to 172 x 172 -- the J
    plane holds real values about a hundred above thresh16 -- and j = -8001 is not; j = -1995 with o = -5 passes that gate with scores
    x16, whose range its lo then leaves: scores x4"""
    sc = (1, 0, 0, 0, -8000)
    l = edge("fit", sc, 2, "square", True)
    assert l == 172 and not admits("fit", sc, l, l, 4, True)[0] and not admits("fit", sc[:4] + (-8001,), l, l, 2, True)[0]
    sites = [l // 3, l // 2]
    uniq = _shape_pairs(l, l, 0x8000)
    c = cells("fitj", sc, uniq, sites)
    thresh = admits("fit", sc, l, l, 2, True)[1]
    assert 0 < 4 * int(c["lo"].min()) - thresh <= 4 * 128, (int(c["lo"].min()), thresh)
    cfg = check(al, "fit", sc, uniq, 12, True, True, sites, ("gate", "jump 8000"))
    assert "packed16 x4 " in cfg, cfg
    cfg = check(al, "fit", sc[:4] + (-8001,), uniq, 12, True, True, sites, ("gate", "jump 8001"))
    assert "int32" in cfg and "packed16" not in cfg, cfg
    sc = (1, -1, -5, -1, -1995)
    assert abs(sc[4] - sc[2]) * 16 <= 32000 and not admits("fit", sc, 100, 140, 4, True)[0] and admits("fit", sc, 100, 140, 2, True)[0]
    cfg = check(al, "fit", sc, _shape_pairs(100, 140, 0x1995), 12, True, True, [40, 90], ("gate", "jump 1995"))
    assert "packed16 x4 " in cfg, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["local", "global"])
def test_gate_two_bit_words_against_byte_words(al, env, mode):
    """scores_fit_byte: |16 m| and |16 u| <= 127 -- m = 7 and u = -7 travel as 2-bit words (score LUT, profile words), m = 8 or
    u = -8 as byte words; each scoring at its own x16 edge"""
    for sc, bits in (((7, -7, -9, -2), 2), ((8, -7, -9, -2), 8), ((7, -8, -9, -2), 8)):
        l = edge(mode, sc, 4, "square")
        uniq = _shape_pairs(l, l, 0xB17E + sc[0])
        for tb in (True, False):
            cfg = check(al, mode, sc, uniq, _even(uniq, batch_size(l)), tb, where=("gate", "bits", mode, sc, tb))
            assert "packed16 x16 bits=%d " % bits in cfg, (sc, cfg)


def _pack2(codes, w):
    """2-bit words of at_pack_batch for every row of a uint8 code array [n, L]: uint32 [n, w], base k in bits 2 k % 32 of word k / 16"""
    n, L = codes.shape
    pad = np.zeros((n, w * 16), dtype=np.uint64)
    pad[:, :L] = codes
    return (pad.reshape(n, w, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=2).astype(np.uint32)


class _DeviceArrays:
    """numpy arrays in device memory through the HIP runtime the shim is linked against (no other package has to start up)"""

    def __init__(self, lib):
        import ctypes as C
        self.C, self.lib, self.ptrs = C, lib, []
        lib.hipMalloc.restype = lib.hipMemcpy.restype = lib.hipFree.restype = lib.hipDeviceSynchronize.restype = C.c_int
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.hipFree.argtypes = [C.c_void_p]

    def up(self, arr):
        p = self.C.c_void_p()
        arr = np.ascontiguousarray(arr)
        assert self.lib.hipMalloc(self.C.byref(p), arr.nbytes + 256) == 0
        self.ptrs.append(p)
        assert self.lib.hipMemcpy(p, arr.ctypes.data_as(self.C.c_void_p), arr.nbytes, 1) == 0    # hipMemcpyHostToDevice
        return p.value

    def down(self, ptr, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.C.c_void_p(ptr), out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.hipFree(p)
        self.ptrs = []


@pytest.mark.gpu
def test_gate_profile_words_against_the_lut_on_the_device_entry(al, env):
    """profile_lookup_ok: (m - u) * 16 <= 255.  2-bit words under 8 / -7 (240: the profile words) and 8 / -8 (256: the score LUT,
    whose 16-bit entries hold 128 and -128) reach the packed local kernels through at_align_batch_device only; each at its x16 edge"""
    import aligntools.c_amd as A
    env.setenv("AT_TWO_PASS", "0")
    dev = _DeviceArrays(A.load_library())
    lut = np.zeros(256, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    try:
        for sc in ((8, -7, -9, -2), (8, -8, -9, -2)):
            l = edge("local", sc, 4, "square")
            assert (sc[0] - sc[1]) * 16 == (240 if sc[1] == -7 else 256) and 209 <= l <= 304
            uniq = _shape_pairs(l, l, 0xDE7 + sc[1])
            n = 72
            pairs = [uniq[k % len(uniq)] for k in range(n)]
            ref = _oracle("local", sc, False, (), uniq)
            codes = lut[np.frombuffer("".join(a + b for a, b in pairs).encode(), dtype=np.uint8)].reshape(n, 2 * l)
            w = (l + 15) // 16 + 1
            d_words = dev.up(np.concatenate([_pack2(codes[:, :l], w), _pack2(codes[:, l:], w)], axis=1))
            base = np.arange(n, dtype=np.int64) * (2 * w)
            d_woff1, d_woff2 = dev.up(base), dev.up(base + w)
            d_len = dev.up(np.full(n, l, dtype=np.int32))
            d_ops_off = dev.up(np.arange(n, dtype=np.int64) * (2 * l))
            al.set_scoring(*sc)
            for tb in (True, False):
                d_ops = dev.up(np.zeros(n * 2 * l + 64, dtype=np.uint8))
                d_res = dev.up(np.zeros(5 * n, dtype=np.int32))
                al.align_batch_device(A.MODE_LOCAL, n, d_words, 2, d_woff1, d_len, d_woff2, d_len, l, l, True, tb, d_res, d_res + 4 * n,
                                      d_res + 8 * n, d_res + 12 * n, d_ops, d_ops_off, d_res + 16 * n, 0)
                h = dev.down(d_res, np.int32, 5 * n).reshape(5, n)
                ops2d = dev.down(d_ops, np.uint8, n * 2 * l).reshape(n, 2 * l)
                cfg = al.last_config
                SEEN.append((("gate", "device entry", sc, tb), cfg))
                assert "packed16 x16 bits=2 " in cfg and GROUPS[16] in cfg, cfg
                for k in range(n):
                    r = ref[k % len(uniq)]
                    assert (int(h[0, k]), int(h[1, k]), int(h[2, k]), int(h[3, k])) == (r["score"], r["end_i"], r["end_j"], r["state"]), (sc, tb, k, cfg)
                    if tb:
                        assert int(h[4, k]) == len(r["ops"]) and ops2d[k, :int(h[4, k])].tobytes() == r["ops"], (sc, k, cfg)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["global", "local", "fit", "overlap"])
def test_gate_exact_range_of_the_int32_kernel(al, env, mode):
    """maxabs * (l1 + l2 + 2) < 2^24 (at_hip.hip :1049): 63 x 63 with every parameter at 131 071 is 2^24 - 128 -- admitted, byte words,
    equal to the fp64 oracle on all-match, nothing-matches and related pairs; 131 072 is refused with AT_ERR_RANGE (-3)"""
    import aligntools.c_amd as A
    v = 131071
    assert v * (63 + 63 + 2) == (1 << 24) - 128
    sc = (v, -v, -v, -v)
    uniq = _shape_pairs(63, 63, 0x1FFFF)
    for tb in (True, False):
        cfg = check(al, mode, sc, uniq, 12, tb, where=("gate", "int32", mode, tb))
        assert "int32 bits=8" in cfg and "packed16" not in cfg, cfg
    if mode in ("global", "local"):
        assert _oracle(mode, sc, False, (), uniq[:1])[0]["score"] == v * 63
    al.set_scoring(v + 1, -v, -v, -v, -10)
    with pytest.raises(A.AlignToolsError) as ei:
        al.align_batch(mode, uniq, traceback=False, render=False)
    assert ei.value.code == -3, ei.value


@pytest.mark.gpu
def test_gate_local_scan_key_and_tile_range(al, env):
    """at_scan_local: mx * l1 < 2^20 (the score field of the key, at_localscan_plan.h :46) -- 1 025 x 1 023 = 2^20 - 1 is admitted,
    and a query that matches its target scores exactly that, the key's top score (field 0); 1 024 x 1 024 = 2^20 is refused.  The tile
    range check maxabs * (l1 + tile + ov + 2) < 2^24 (at_hip.hip :2911): tiles of 13 280 columns are the last admitted, 13 296 are
    refused.  Every admitted run equals search("local") and the oracle."""
    import aligntools.c_amd as A
    m, l1 = 1025, 1023
    assert m * l1 == (1 << 20) - 1
    sc = (m, -m, -m, -m)
    ov = (l1 + (m * l1 - 1) // m + 15) & ~15                 # localscan_overlap: pen = 1 025
    tile = max(t for t in range(16, 1 << 15, 16) if m * (l1 + t + ov + 2) < 1 << 24)
    assert (ov, tile) == (2048, 13280) and m * (l1 + tile + 16 + ov + 2) >= 1 << 24
    rng = random.Random(0x5CA7)
    q = _rnd(rng, l1)
    other = _rnd(rng, l1)
    target = _rnd(rng, 9000) + q + _rnd(rng, 14900 - 9000 - l1)
    assert m * (l1 + len(target) + 2) < 1 << 24                # (search("local") sweeps the whole target as one pair)
    al.set_scoring(*sc, -10)
    want = al.search("local", [q, other], [target], k=1)
    SEEN.append((("gate", "scan search"), al.last_config))
    for t in (0, tile):
        got = al.scan_local([q, other], [target], k=1, tile_cols=t)
        SEEN.append((("gate", "scan_local", t), al.last_config))
        for name in ("score", "end_i", "end_j", "state", "target"):
            assert (got[name] == want[name]).all(), (t, name, got[name], want[name])
    assert int(want["score"][0, 0]) == (1 << 20) - 1 and (int(want["end_i"][0, 0]), int(want["end_j"][0, 0])) == (l1, 9000 + l1)
    for k, s in enumerate((q, other)):
        r = _oracle("local", sc, False, (), [(s, target)])[0]
        assert (int(want["score"][k, 0]), int(want["end_i"][k, 0]), int(want["end_j"][k, 0])) == (r["score"], r["end_i"], r["end_j"]), k
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_local([q], [target], k=1, tile_cols=tile + 16)
    assert ei.value.code == -3 and "exact score range" in str(ei.value), ei.value
    al.set_scoring(1024, -1024, -1024, -1024, -10)
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_local([q + "A"], [target], k=1)
    assert ei.value.code == A.ERR_DOMAIN, ei.value


@pytest.mark.gpu
def test_baseline_shapes_keep_their_engines(al, env):
    """the shapes and scorings of bench.py's C2 .. C5 on the engines they have had: scores x16 for C2 and C4, x4 for C3 and C5"""
    for name, mode, l1, l2, sc, uj, sites, want in (("C2", "local", 150, 150, (2, -2, -5, -2), False, [], "packed16 x16 "),
                                                    ("C3", "global", 1024, 1024, (1, -1, -4, -1), False, [], "packed16 x4 "),
                                                    ("C4", "fit", 150, 500, (2, -2, -5, -1, -10), True, [100, 200, 300, 400], "packed16 x16 "),
                                                    ("C5", "overlap", 1000, 1000, (1, -2, -5, -1), False, [], "packed16 x4 ")):
        uniq = _shape_pairs(l1, l2, _seed(name), 2)
        cfg = check(al, mode, sc, uniq, len(uniq), True, uj, sites, ("baseline", name))
        assert want in cfg, (name, cfg)


@pytest.mark.gpu
def test_every_family_was_seen():
    """the launches of this module, by last_config: every kernel family and both sides of every gate"""
    cfgs = [c for _, c in SEEN]
    if not cfgs:
        pytest.skip("runs behind the other tests of this module")

    def seen(*texts, tag=None):
        return any(all(t in c for t in texts) and (tag is None or (w and w[0] == tag)) for w, c in SEEN)
    missing = []
    for g in (4, 8, 16, 32, 64):
        for bits in (2, 8) if g != 32 else (2,):
            if not seen("packed16 x16 bits=%d" % bits, GROUPS[g]):
                missing.append(("x16", g, bits))
    for text in ("rows/lane=4 ", "rows/lane=16 "):
        for bits in (2, 8):
            if not seen("packed16 x4 bits=%d" % bits, text):
                missing.append(("x4", text, bits))
    for g, rows in ((8, 19), (64, 16)):
        for text in ("two-pass ck=", "two-pass (walk kernel)", "teams"):
            if not seen("packed16 x16 ", GROUPS[g], text, "rows/lane=%d " % rows):
                missing.append(("two-pass x16", g, text))
    for text in ("two-pass ck=", "two-pass (walk kernel)", "teams"):
        if not seen("packed16 x4 ", text):
            missing.append(("two-pass x4", text))
    for g in (8, 32, 64):
        if not seen("packed16", "ragged frames", GROUPS[g], tag="ragged"):
            missing.append(("ragged", g))
    for tag in ("flip", "family", "ragged", "gate", "baseline"):
        if not seen("", tag=tag):
            missing.append(("part", tag))
    if not seen("int32 bits=8", tag="gate") or not seen("int32 bits=2"):
        missing.append("int32")
    assert not missing, missing


if __name__ == "__main__":
    print("%-42s %-10s %-8s %5s %8s %8s %8s  %s" % ("case", "shape", "group", "bits", "thresh16", "reach_hi", "reach_lo", "one base further"))
    for c in CASES:
        rh, rl, _ = reach(c)
        print("%-42s %-10s %-8s %5d %8d %8d %8d  %s" % (c.id, "%dx%d" % (c.l1, c.l2), "%d lanes" % c.g, c.bits, c.thresh16, rh, rl, c.engine(1)), flush=True)
