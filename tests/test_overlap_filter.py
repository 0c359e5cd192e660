"""The overlap filter (at_set_min_score; at_myers<W, 1, true> in csrc/at_myers.hip.h) held to the VALUE of its bound.

The filter reports, for every pair it does not hand to the exact sweep, an upper bound of the overlap score.  That bound has an
exact definition: with D'(i, j) the unit-cost edit distance with a free start in s1 -- D'(i, 0) = 0, D'(0, j) = j --
over s1 left-padded with 'A' (code 0) to the 32 W rows of its word class,

    ub = max(0, max over 1 <= b <= l2 - 1 of 2 m b - k2 D'(32 W, b)) >> 1,        k2 = min(2 (m - u), m - 2 o) - m,

and a pair is swept iff ub >= T.  The reference below is that definition as plain DP (ub_scalar) and the same thing vectorised over
the pairs of a triangle (ub_triangle).  The CPU half checks the two against each other, the inequality ub(padded) >= ub(unpadded) >=
overlap score of the oracle, and conditions on the read sets that keep the GPU half meaningful whatever the seeds: pairs on both
sides of a threshold in every word class, pairs whose bound is tight, pairs whose last column decides.  The GPU half runs two read
sets per word class (2, 3, 4, 5, 8, 16, 32 words per lane; one up to the class maximum, one just above the class below it) under
every scoring and threshold and compares every pair of the triangle: stopped pairs carry exactly ub, swept pairs exactly the
unthresholded results, which equal the oracle.  All comparisons are equalities of integers."""
import functools
import random
import re

import numpy as np
import pytest

import aligntools.c_amd as A
import oracle as O

DEFAULT = (1, -2, -5, -1)
ELIGIBLE = [DEFAULT,                 # k2 = 5, odd: the halving matters
            (2, -3, -4, -1),         # k2 = 8
            (3, -1, -2, -1)]         # k2 = 4: the gap term is the minimum
ZERO_MATCH = (0, -1, -1, -1)         # k2 = 2, m = 0: eligible (m >= 0), every bound is 0
INELIGIBLE = [(2, 1, -1, -1), (1, -2, 0, -1)]     # k2 = 0: no filter
WORDS = (2, 3, 4, 5, 8, 16, 32)
CLASS_MAX = {2: 64, 3: 96, 4: 128, 5: 160, 8: 256, 16: 512, 32: 1024}
LOW_EDGE = {2: 33, 3: 65, 4: 97, 5: 129, 8: 161, 16: 257, 32: 513}
NREADS = {2: 40, 3: 40, 4: 40, 5: 40, 8: 40, 16: 24, 32: 16}
LOW_ALPHABET = {2: "AAAC", 3: "CGT", 4: "AAAC", 5: "CGT", 8: "AAAC", 16: "CGT", 32: "AAAC"}   # A-rich: the pad rows match; no A: they never do
SEEDS = {(32, "full"): 1, (32, "low"): 4}    # where the default seed (read_set) misses coverage condition (b): four planted pairs, three must be tight
SET_KEYS = [(w, kind) for w in WORDS for kind in ("full", "low")]
SET_IDS = ["w%d-%s" % k for k in SET_KEYS]
EXTREME_T = (-(2 ** 31), 0, 2 ** 30, 2 ** 31 - 1)      # T <= 0: every pair is swept; 2 T beyond int32: none is


def k2_of(m, u, o):
    return min(2 * (m - u), m - 2 * o) - m


# ---------------------------------------------------------------- read sets
def set_lengths(W, kind):
    """The lengths of a set: 1, 2, 15, 16, 17, 31, 32, 33, every multiple of 32 with its two neighbours and the maximum, where they
    fit; the rest drawn from 1 .. maximum.  The classes of 16 and 32 words have more such lengths (50 and 98) than reads (24 and 16):
    there the set keeps the small lengths, the maximum and the one below it, the last length of the class below with its neighbours
    (255 .. 257 / 511 .. 513), and of every other multiple of 32 one of (k - 1, k, k + 1) in turn, evenly spread over the class."""
    mx = CLASS_MAX[W] if kind == "full" else LOW_EDGE[W]
    n = NREADS[W]
    rng = random.Random(1000 * W + (kind == "low"))
    small = [x for x in (1, 2, 15, 16, 17, 31, 32, 33) if x <= mx]
    mult = list(range(32, mx + 1, 32))
    must = small + [x for k in mult for x in (k - 1, k, k + 1) if x <= mx] + [mx]
    must = sorted(set(must))
    if len(must) > n:
        below = LOW_EDGE[W] - 1
        must = sorted(set(small + [mx, mx - 1] + [x for x in (below - 1, below, below + 1) if x <= mx]))
        rest = [k for k in mult if k > 33 and not {k - 1, k, k + 1} & set(must)]
        room = min(n - len(must), len(rest))
        for q in range(room):
            must.append(rest[int((q + 0.5) * len(rest) / room)] + (q % 3) - 1)
    lens = must + [rng.randint(1, mx) for _ in range(n - len(must))]
    assert len(lens) == n and len(set(must)) == len(must) and max(lens) == mx and min(lens) >= 1
    return lens


@functools.lru_cache(maxsize=None)
def read_set(W, kind):
    """(reads, exact, suffix): the reads of a set, the pairs (k - 1, k) where read k starts with an exact copy of a suffix of read
    k - 1 (every fourth read), and the one pair where read k is wholly a suffix of read k - 1.  Every other fourth read starts with a
    noisy copy -- substitutions, insertions, deletions -- of such a suffix.  Lengths are those of set_lengths, shuffled."""
    alpha = "ACGT" if kind == "full" else LOW_ALPHABET[W]
    rng = random.Random(SEEDS.get((W, kind), 7 * W + (kind == "low")))
    lens = set_lengths(W, kind)
    rng.shuffle(lens)
    n = len(lens)
    dna = lambda k: "".join(rng.choice(alpha) for _ in range(k))
    # the read that is wholly a suffix of its predecessor: the longest candidate among the reads with an exact copy
    ks = max(range(1, n, 4), key=lambda k: lens[k] if lens[k] <= lens[k - 1] else -1)
    if lens[ks] > lens[ks - 1]:
        lens[ks], lens[ks - 1] = lens[ks - 1], lens[ks]
    reads = [dna(k) for k in lens]
    exact = []
    for k in range(1, n):
        prev, cur = reads[k - 1], reads[k]
        most = min(len(prev), len(cur))
        if k == ks:
            reads[k] = prev[len(prev) - len(cur):]
            exact.append((k - 1, k))
        elif k % 4 == 1:
            ov = rng.randint(min(most, 8), most)
            reads[k] = prev[len(prev) - ov:] + cur[ov:]
            exact.append((k - 1, k))
        elif k % 4 == 3:
            ov = rng.randint(min(most, 8), most)
            piece = list(prev[len(prev) - ov:])
            for _ in range(ov // 12 + 1):
                q = rng.randrange(len(piece))
                r = rng.random()
                if r < 0.5:
                    piece[q] = rng.choice(alpha)
                elif r < 0.75 and len(piece) > 1:
                    del piece[q]
                else:
                    piece.insert(q, rng.choice(alpha))
            reads[k] = ("".join(piece) + cur[ov:] + cur)[:len(cur)]
    assert [len(r) for r in reads] == lens
    return tuple(reads), tuple(exact), (ks - 1, ks)


def tri_index(n, a, b):
    """Index of the pair a < b in the triangle order of all-vs-all (row by row)."""
    return a * n - a * (a + 1) // 2 + (b - a - 1)


# ---------------------------------------------------------------- the reference
def ub_scalar(s1, s2, m, u, o, W=None, limit=None):
    """The bound of one pair by plain DP.  W: s1 is left-padded with 'A' to 32 W rows (what the kernel computes); None: s1 as it
    is (what DESIGN 3.7 derives).  limit: the last column b that counts, l2 - 1 unless given."""
    if W is not None:
        assert len(s1) <= 32 * W
        s1 = "A" * (32 * W - len(s1)) + s1
    last = _last_row_scalar(s1, s2)
    k2 = k2_of(m, u, o)
    ub2 = 0
    for b in range(1, (len(s2) - 1 if limit is None else limit) + 1):
        ub2 = max(ub2, 2 * m * b - k2 * last[b])
    return ub2 >> 1


@functools.lru_cache(maxsize=4096)
def _last_row_scalar(s1, s2):
    """D'(l1, b), b = 0 .. l2: cell by cell (kept per pair of strings: the scorings share it)."""
    l1, l2 = len(s1), len(s2)
    D = [[0] * (l2 + 1) for _ in range(l1 + 1)]
    for j in range(l2 + 1):
        D[0][j] = j
    for i in range(1, l1 + 1):
        row, above, c = D[i], D[i - 1], s1[i - 1]
        for j in range(1, l2 + 1):
            best = above[j - 1] + (c != s2[j - 1])
            for other in (above[j] + 1, row[j - 1] + 1):
                if other < best:
                    best = other
            row[j] = best
    return tuple(D[l1])


_CODE = np.full(256, 255, dtype=np.uint8)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k


def last_rows(reads, W):
    """D'(rows, b), b = 0 .. l2, of every pair a < b of `reads` in triangle order, as an int16 array (pairs, longest + 1); entries
    beyond a pair's l2 mean nothing.  Column by column over all pairs at once: with N(i) = min(D'(i - 1, j - 1) + (s1[i] != s2[j]),
    D'(i, j - 1) + 1) and N(0) = j, the column is min over i' <= i of (N(i') - i') + i.  W = None pads s1 to the longest read with a
    symbol that matches nothing, which leaves D' as it is without padding: a free start skips rows at no cost, and a row that
    matches nothing is never worth using."""
    n = len(reads)
    lens = np.array([len(r) for r in reads])
    rows = 32 * W if W is not None else int(lens.max())
    cols = int(lens.max())
    S1 = np.full((n, rows), 0 if W is not None else 254, dtype=np.uint8)
    S2 = np.full((n, cols), 253, dtype=np.uint8)
    for k, r in enumerate(reads):
        c = _CODE[np.frombuffer(r.encode(), dtype=np.uint8)]
        assert (c < 4).all()
        S1[k, rows - len(r):] = c
        S2[k, :len(r)] = c
    ia, ib = np.triu_indices(n, 1)
    X, Y = S1[ia], S2[ib]
    ar = np.arange(rows + 1, dtype=np.int16)
    prev = np.zeros((len(ia), rows + 1), dtype=np.int16)
    out = np.zeros((len(ia), cols + 1), dtype=np.int16)
    N = np.empty_like(prev)
    for j in range(1, cols + 1):
        N[:, 0] = j
        np.minimum(prev[:, :-1] + (X != Y[:, j - 1:j]), prev[:, 1:] + 1, out=N[:, 1:])
        N -= ar
        np.minimum.accumulate(N, axis=1, out=prev)
        prev += ar
        out[:, j] = prev[:, -1]
    return out, lens[ib]


@functools.lru_cache(maxsize=None)
def _set_last_rows(W, kind, pad_words):
    return last_rows(read_set(W, kind)[0], pad_words)


def bound_from_rows(D, l2, m, u, o, limit_l2=False):
    b = np.arange(D.shape[1], dtype=np.int64)
    val = 2 * m * b[None, :] - k2_of(m, u, o) * D.astype(np.int64)
    last = l2 if limit_l2 else l2 - 1
    val[(b[None, :] < 1) | (b[None, :] > last[:, None])] = 0
    return val.max(axis=1) >> 1


def ub_triangle(reads, m, u, o, W):
    """ub_scalar for every pair a < b of `reads`, in triangle order."""
    D, l2 = last_rows(reads, W)
    return bound_from_rows(D, l2, m, u, o)


def set_bounds(key, sc, pad_words, limit_l2=False):
    """ub_triangle of a read set of this module, memoised per (set, padding): the DP does not depend on the scoring."""
    D, l2 = _set_last_rows(key[0], key[1], pad_words)
    return bound_from_rows(D, l2, sc[0], sc[1], sc[2], limit_l2)


@functools.lru_cache(maxsize=None)
def oracle_triangle(key, sc):
    """score / end_i / end_j / state of the oracle's overlap alignment of every pair of a set, (4, pairs) in triangle order."""
    reads = read_set(*key)[0]
    return _oracle_rows(reads, sc)


def _oracle_rows(reads, sc):
    n = len(reads)
    out = np.zeros((4, n * (n - 1) // 2), dtype=np.int64)
    enc = [r.encode() for r in reads]
    q = 0
    for a in range(n):
        for b in range(a + 1, n):
            r = O.align(O.OVERLAP, enc[a], enc[b], *sc)
            assert r["rc"] == 0
            out[:, q] = (r["score"], r["end_i"], r["end_j"], r["state"])
            q += 1
    out.setflags(write=False)
    return out


def planted_threshold(key, sc):
    """v of the thresholds v, v + 1: the bound of a planted exact pair -- the smallest one of at least 4, to keep it near the crowd."""
    reads, exact, _ = read_set(*key)
    ub = set_bounds(key, sc, key[0])
    vs = sorted(int(ub[tri_index(len(reads), a, b)]) for a, b in exact)
    big = [v for v in vs if v >= 4]
    return big[0] if big else vs[-1]


def thresholds(key, sc):
    v = planted_threshold(key, sc)
    return [10 ** 6, 1, 2, 3, v, v + 1]


# ---------------------------------------------------------------- CPU half
def test_read_sets_have_the_stated_lengths_and_alphabets():
    for W, kind in SET_KEYS:
        reads, exact, (sa, sb) = read_set(W, kind)
        mx = CLASS_MAX[W] if kind == "full" else LOW_EDGE[W]
        lens = [len(r) for r in reads]
        assert len(reads) == NREADS[W] and max(lens) == mx and min(lens) >= 1
        want = [x for x in (1, 2, 15, 16, 17, 31, 32, 33) if x <= mx] + [mx]
        if W <= 8:
            want += [x for k in range(32, mx + 1, 32) for x in (k - 1, k, k + 1) if x <= mx]
        else:
            want += [mx - 1, LOW_EDGE[W] - 2, LOW_EDGE[W] - 1] + ([LOW_EDGE[W]] if LOW_EDGE[W] <= mx else [])
            near = {k for k in range(64, mx + 1, 32) if {k - 1, k, k + 1} & set(lens)}
            assert len(near) >= min(NREADS[W] - 13, len(range(64, mx + 1, 32))), (W, kind, sorted(near))
            assert {x % 32 for x in lens if x > 33} >= {31, 0, 1}
        assert set(want) <= set(lens), (W, kind, sorted(set(want) - set(lens)))
        assert set("".join(reads)) <= set("ACGT" if kind == "full" else LOW_ALPHABET[W])
        assert reads[sa].endswith(reads[sb]) and (sa, sb) in exact
        assert len(exact) == len(range(1, len(reads), 4))
        for a, b in exact:
            assert any(reads[a].endswith(reads[b][:k]) for k in range(min(8, len(reads[a]), len(reads[b])), len(reads[b]) + 1))


def _scalar_sample(key):
    """Pairs of a set for the scalar DP, as (a, b): a fixed number of cheap ones, spread over the triangle, and two larger ones."""
    reads = read_set(*key)[0]
    n = len(reads)
    rng = random.Random(key[0] * 2 + (key[1] == "low"))
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    cost = lambda p: 32 * key[0] * len(reads[p[1]])
    cheap = [p for p in pairs if cost(p) <= 40000]
    mid = [p for p in pairs if 40000 < cost(p) <= 200000]
    return rng.sample(cheap, min(22, len(cheap))) + rng.sample(mid, min(2, len(mid)))


@pytest.mark.parametrize("key", SET_KEYS, ids=SET_IDS)
def test_vectorised_reference_equals_scalar_dp(key):
    """ub_triangle against ub_scalar on pairs of every set, padded and unpadded, under every eligible scoring (at least 300 pairs over
    the sets: the count is asserted in test_scalar_sample_is_large_enough)."""
    reads = read_set(*key)[0]
    n = len(reads)
    for W in (key[0], None):
        for a, b in _scalar_sample(key):
            for sc in ELIGIBLE + [ZERO_MATCH]:
                want = ub_scalar(reads[a], reads[b], *sc[:3], W=W)
                assert int(set_bounds(key, sc, W)[tri_index(n, a, b)]) == want, (key, W, a, b, sc)
            want = ub_scalar(reads[a], reads[b], *DEFAULT[:3], W=W, limit=len(reads[b]))
            assert int(set_bounds(key, DEFAULT, W, limit_l2=True)[tri_index(n, a, b)]) == want, (key, W, a, b)


def test_scalar_sample_is_large_enough():
    assert sum(len(_scalar_sample(key)) for key in SET_KEYS) >= 300


def test_ub_triangle_on_a_plain_list():
    """The public form, on reads that are not one of the sets: every pair against the scalar DP."""
    rng = random.Random(3)
    reads = ["".join(rng.choice("AC") for _ in range(rng.randint(1, 40))) for _ in range(12)]
    for W in (2, None):
        got = ub_triangle(reads, 1, -2, -5, W)
        want = [ub_scalar(reads[a], reads[b], 1, -2, -5, W=W) for a in range(12) for b in range(a + 1, 12)]
        assert got.tolist() == want


@pytest.mark.parametrize("key", SET_KEYS, ids=SET_IDS)
def test_bound_inequality_on_every_pair(key):
    """ub(s1 padded with 'A' to the class's rows) >= ub(s1 as it is) >= the oracle's overlap score, on every pair of
    every set under every eligible scoring; without an A in the reads the pad rows match nothing and the two bounds coincide."""
    for sc in ELIGIBLE + [ZERO_MATCH]:
        padded, plain = set_bounds(key, sc, key[0]), set_bounds(key, sc, None)
        score = oracle_triangle(key, sc)[0]
        assert (padded >= plain).all() and (plain >= score).all(), (key, sc)
        if key[1] == "low" and "A" not in LOW_ALPHABET[key[0]]:
            assert (padded == plain).all(), (key, sc)
        if sc[0] == 0:
            assert (padded == 0).all() and (score == 0).all()


def test_bound_inequality_exhaustive_on_short_strings():
    """Every ordered pair of strings over {A, C} of length 1 .. 4: l2 = 1 (no column counts: the bound is 0), b <= l2 - 1, pad rows
    that match."""
    strings = ["".join("AC"[(v >> k) & 1] for k in range(n)) for n in range(1, 5) for v in range(1 << n)]
    assert len(strings) == 30
    for sc in ELIGIBLE + [ZERO_MATCH]:
        grew = 0
        for s1 in strings:
            for s2 in strings:
                padded, plain = ub_scalar(s1, s2, *sc[:3], W=2), ub_scalar(s1, s2, *sc[:3])
                score = O.align(O.OVERLAP, s1, s2, *sc)["score"]
                assert padded >= plain >= score, (sc, s1, s2, padded, plain, score)
                if len(s2) == 1:
                    assert padded == 0 and score == 0
                if "A" not in s2:
                    assert padded == plain
                grew += padded > plain
        assert (grew > 0) == (sc[0] > 0), sc                         # the pad rows do raise some bounds


def _on_both_sides(ub, T):
    return int((ub == T).sum()) >= 3 and int((ub == T - 1).sum()) >= 3


@pytest.mark.parametrize("W", WORDS)
def test_coverage_pairs_on_both_sides_of_a_threshold(W):
    """(a) For every word class, under the default scoring, some threshold of the list has at least three pairs whose bound equals it
    (swept) and three one below (stopped): `>=` turned into `>`, or a bound off by one, changes the swept set.  Held on both sets."""
    for kind in ("full", "low"):
        ub = set_bounds((W, kind), DEFAULT, W)
        assert any(_on_both_sides(ub, T) for T in thresholds((W, kind), DEFAULT)[1:]), (W, kind, np.bincount(ub)[:8].tolist())


@pytest.mark.parametrize("key", SET_KEYS, ids=SET_IDS)
def test_coverage_tight_bounds_and_last_column(key):
    """(b) At least three planted exact overlaps whose bound equals their oracle score (a bound below it would lose a real overlap;
    these pairs have no slack).  (c) At least one pair whose second read is wholly a suffix of the first, so that the column limit
    l2 - 1 and the limit l2 give different bounds."""
    reads, exact, (sa, sb) = read_set(*key)
    n = len(reads)
    ub, score = set_bounds(key, DEFAULT, key[0]), oracle_triangle(key, DEFAULT)[0]
    tight = [p for p in exact if ub[tri_index(n, *p)] == score[tri_index(n, *p)] and score[tri_index(n, *p)] > 0]
    assert len(tight) >= 3, (key, [(int(ub[tri_index(n, *p)]), int(score[tri_index(n, *p)])) for p in exact])
    to_l2 = set_bounds(key, DEFAULT, key[0], limit_l2=True)
    q = tri_index(n, sa, sb)
    assert reads[sa].endswith(reads[sb]) and to_l2[q] != ub[q] and to_l2[q] == len(reads[sb]), (key, int(ub[q]), int(to_l2[q]))


# ---------------------------------------------------------------- GPU half
@pytest.fixture(scope="module")
def al():
    a = A.Aligner(0)
    yield a
    a.set_min_score(None)
    a.close()


class _Device:
    """A read set packed on the device, and the all-vs-all overlap entry over it."""

    def __init__(self, reads):
        import torch
        self.torch = torch
        self.reads = reads
        self.n = len(reads)
        self.total = self.n * (self.n - 1) // 2
        words, woff, _w2, lens, _l2, self.bits = A.pack_pairs([(r.encode(), b"") for r in reads])
        self.dev = torch.device("cuda", 0)
        self.words = torch.from_numpy(words.view(np.int32)).to(self.dev)
        self.woff = torch.from_numpy(woff).to(self.dev)
        self.len = torch.from_numpy(lens).to(self.dev)
        self.maxl = int(lens.max())

    def sweep(self, al, first=0, npairs=None, slots=None, at=0, fill=-7):
        """Pairs [first, first + npairs) of the triangle into slots [at, at + npairs) of a (4, slots) tensor pre-filled with `fill`."""
        torch = self.torch
        npairs = self.total if npairs is None else npairs
        res = torch.full((4, npairs if slots is None else slots), fill, dtype=torch.int32, device=self.dev)
        al.align_allpairs_device(A.MODES["overlap"], self.n, self.words.data_ptr(), self.bits, self.woff.data_ptr(), self.len.data_ptr(),
                                 self.maxl, first, npairs, False, res[0, at:].data_ptr(), res[1, at:].data_ptr(), res[2, at:].data_ptr(),
                                 res[3, at:].data_ptr(), 0, 0, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return res.cpu().numpy().astype(np.int64)


_devices = {}


def device_set(key):
    if key not in _devices:
        _devices[key] = _Device(read_set(*key)[0])
    return _devices[key]


FILTER_NOTE = re.compile(r"overlap filter \(bit-parallel bound, (\d+) words/lane, min score (-?\d+)\)")


def thresholded(al, dev, T, **kw):
    """(results, words per lane named by at_last_config) of a sweep with the threshold T; the threshold is off again afterwards."""
    al.set_min_score(T)
    try:
        got = dev.sweep(al, **kw)
    finally:
        al.set_min_score(None)
    note = FILTER_NOTE.search(al.last_config)
    assert note and int(note.group(2)) == T, al.last_config
    return got, int(note.group(1))


def check_against_reference(got, exact, ub, T, tag):
    """The contract of include/aligntools_hip.h with the bound's value: a pair is swept iff its bound reaches T; a stopped pair
    reports (bound, l1 untested, 0, 0), a swept one what the unthresholded sweep reports."""
    swept = got[3] == 2
    assert ((got[3] == 0) | swept).all(), tag
    assert (swept == (ub >= T)).all(), (tag, np.flatnonzero(swept != (ub >= T))[:8].tolist())
    stopped = ~swept
    assert (got[0][stopped] == ub[stopped]).all(), (tag, np.flatnonzero(stopped & (got[0] != ub))[:8].tolist())
    assert (got[2][stopped] == 0).all() and (got[3][stopped] == 0).all(), tag
    assert (got[:, swept] == exact[:, swept]).all(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("key", SET_KEYS, ids=SET_IDS)
def test_filter_equals_reference(al, key):
    """Every pair of the set, every eligible scoring, the thresholds 10^6 (nothing swept: every pair reports its bound), 1, 2, 3 and
    v, v + 1 around a planted exact pair's bound: the class named by at_last_config is the set's, the unthresholded sweep equals the
    oracle, and the thresholded one equals the reference bound / the unthresholded sweep pair by pair.  One set also runs m = 0 and
    the thresholds at the ends of int32."""
    dev = device_set(key)
    assert dev.bits == 2
    for sc in ELIGIBLE + ([ZERO_MATCH] if key == (5, "full") else []):
        al.set_scoring(*sc)
        al.set_min_score(None)
        exact = dev.sweep(al)
        assert "filter" not in al.last_config, al.last_config
        assert (exact == oracle_triangle(key, sc)).all(), (key, sc)
        for T in thresholds(key, sc) + (list(EXTREME_T) if key in ((3, "low"), (5, "full")) else []):
            got, words = thresholded(al, dev, T)
            assert words == key[0], (key, al.last_config)
            ub = set_bounds(key, sc, words)
            check_against_reference(got, exact, ub, T, (key, sc, T))
            if T == 10 ** 6 or T >= 2 ** 30:
                assert (got[3] == 0).all() and (got[0] == ub).all()
            if T <= 0:
                assert (got[3] == 2).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sc", INELIGIBLE, ids=["m2u1o-1", "m1u-2o0"])
def test_ineligible_scorings_sweep_every_pair(al, sc):
    """k2 = 0 (2 c = m): the bound says nothing, no filter runs, every pair is swept and equals the oracle."""
    assert k2_of(*sc[:3]) == 0
    for key in ((4, "low"), (16, "full")):
        dev = device_set(key)
        al.set_scoring(*sc)
        al.set_min_score(2)
        try:
            got = dev.sweep(al)
        finally:
            al.set_min_score(None)
        assert "filter" not in al.last_config, al.last_config
        assert (got == oracle_triangle(key, sc)).all() and (got[3] == 2).all(), (key, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(3, "full"), (8, "low")], ids=["w3-full", "w8-low"])
def test_window_of_the_triangle(al, key):
    """first_pair = 37, npairs = 300 of the 780 pairs, written into the middle of larger tensors: the slots outside the window keep
    their sentinel, the window equals the same slice of the full run (bounds and exact results alike)."""
    dev = device_set(key)
    al.set_scoring(*DEFAULT)
    for T in (2, 10 ** 6):
        full, words = thresholded(al, dev, T)
        assert words == key[0]
        part, words = thresholded(al, dev, T, first=37, npairs=300, slots=500, at=100, fill=-77)
        assert words == key[0]
        assert (part[:, :100] == -77).all() and (part[:, 400:] == -77).all()
        assert (part[:, 100:400] == full[:, 37:337]).all()
        check_against_reference(part[:, 100:400], oracle_triangle(key, DEFAULT)[:, 37:337], set_bounds(key, DEFAULT, words)[37:337], T, (key, T))


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(4, "full"), (16, "low")], ids=["w4-full", "w16-low"])
def test_stream_with_threshold_equals_one_shot(al, key):
    """at_align_allpairs_stream with a threshold in slices of 97 pairs: identical to the one-shot device run, slice by slice."""
    dev = device_set(key)
    reads = dev.reads
    blob = np.frombuffer("".join(reads).encode() + b"\0", dtype=np.uint8).copy()
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    off = np.zeros(len(reads), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    al.set_scoring(*DEFAULT)
    for T in (2, planted_threshold(key, DEFAULT)):
        one, words = thresholded(al, dev, T)
        got = np.full((4, dev.total), -7, dtype=np.int64)
        firsts = []

        def on_slice(first, sc, ei, ej, st):
            firsts.append((first, len(sc)))
            for row, x in enumerate((sc, ei, ej, st)):
                got[row, first:first + len(x)] = x
        al.set_min_score(T)
        try:
            al.align_allpairs_stream("overlap", blob, off, lens, 0, dev.total, 97, on_slice)
        finally:
            al.set_min_score(None)
        note = FILTER_NOTE.search(al.last_config)
        assert note and int(note.group(1)) == key[0] == words and "slices" in al.last_config, al.last_config
        assert firsts == [(f, min(97, dev.total - f)) for f in range(0, dev.total, 97)]
        assert (got == one).all(), (key, T)
        check_against_reference(got, oracle_triangle(key, DEFAULT), set_bounds(key, DEFAULT, words), T, (key, T))


@pytest.mark.gpu
def test_handle_reuse_across_classes(al):
    """One handle: a thresholded call on 276 pairs, the threshold switched off (every pair swept, no filter named), a thresholded call
    on a set of another class with 780 pairs (the candidate list grows, its counter starts from 0), and the first set again."""
    al.set_scoring(*DEFAULT)
    small, large = (16, "full"), (8, "full")
    for key in (small, large, small):
        dev = device_set(key)
        got, words = thresholded(al, dev, 2)
        assert words == key[0]
        exact = dev.sweep(al)                                         # (thresholded() switched the threshold off)
        assert "filter" not in al.last_config and (exact[3] == 2).all(), al.last_config
        assert (exact == oracle_triangle(key, DEFAULT)).all()
        check_against_reference(got, exact, set_bounds(key, DEFAULT, words), 2, key)


@pytest.mark.gpu
def test_no_filter_for_byte_sets_and_long_reads(al):
    """A threshold on sets the filter does not take -- one N in one read (8-bit codes), a longest read of 1 025 bases -- names no
    filter, sweeps every pair and equals the oracle."""
    al.set_scoring(*DEFAULT)
    reads = list(read_set(3, "full")[0])
    k = max(range(len(reads)), key=lambda k: len(reads[k]))
    reads[k] = reads[k][:40] + "N" + reads[k][41:]
    rng = random.Random(1025)
    long_set = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (1025, 1024, 700, 64, 33, 1, 300, 1000)]
    long_set[3] = long_set[0][-64:]
    for case, bits in ((reads, 8), (long_set, 2)):
        dev = _Device(tuple(case))
        assert dev.bits == bits
        al.set_min_score(2)
        try:
            got = dev.sweep(al)
        finally:
            al.set_min_score(None)
        assert "filter" not in al.last_config, al.last_config
        assert (got[3] == 2).all() and (got == _oracle_rows(case, DEFAULT)).all()
