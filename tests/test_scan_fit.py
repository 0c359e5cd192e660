"""at_scan_fit / Aligner.scan_fit: end-to-end affine alignment of reads against long targets.

Nothing new is defined: a hit is what align_batch("fit") returns without jump sites for (query or its reverse complement, whole
target), so every expected value is oracle.align(FIT, ...) on the whole target, ranked by the rule of at_search_strands; a target
shorter than the query is no candidate.

On the CPU: the exports, the plan's values at hand-computed points, the Python-side argument errors and the two facts that make the
tiling exact -- the tile fact (with and without a cutoff) and the window fact -- as a pure Python driver over oracle.align with the
planner's own numbers, plus a control with an overlap of 16 columns that must go wrong.  On the GPU every hit is compared in full."""
import random

import numpy as np
import pytest

import aligntools.c_amd as A
import oracle as O

FIT = O.MODE_NAMES["fit"]
TRUNC = (2, -6, -2, -1)                                         # mismatches cost more than a closing gap row: hits end in state LOW
SCORINGS = [(2, -2, -5, -2), (1, -2, -5, -1), (5, -4, -10, -1), TRUNC]
CPU_SCORINGS = [(2, -2, -5, -2), (1, -2, -5, -1), (5, -4, -10, -1), (3, -1, -1, -3), (1, -1, -2, -2), (4, 1, -3, -1)]
NAMES = ("target", "score", "end_i", "end_j", "state", "nhits")
STRANDS_OF = {"forward": (0,), "reverse": (1,), "both": (0, 1)}


def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _rc(s):
    return A.revcomp(s).decode("latin1")


def _fit(q, t, sc):
    r = O.align(FIT, q, t, sc[0], sc[1], sc[2], sc[3])
    assert r["rc"] == 0, (len(q), len(t), r["rc"])
    return r


def _hit(r):
    return (r["score"], r["state"], r["end_j"])


@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


# ---------------------------------------------------------------- CPU: exports, the planner's export, argument errors

def test_symbols_exported(lib):
    for name in ("at_scan_fit", "at_scan_fit_plan", "at_scan_fit_window"):
        assert name in A.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(A.Aligner.scan_fit) and callable(A.scan_fit_plan) and callable(A.scan_fit_window)


def test_plan_export(lib):
    # 150 rows, 2/-2/-5/-2: lb = -300 - 7, g = floor((300 + 307) / 2) = 303, ov = round16up(150 + 303 + 1) = 464
    assert A.scan_fit_plan(150, 300000, 2, -2, -5, -2) == (1024, 464, 293, 292)
    # a cutoff of 150: g = 75, ov = round16up(226) = 240; one under lb changes nothing
    assert A.scan_fit_plan(150, 300000, 2, -2, -5, -2, min_score=150) == (1024, 240, 293, 292)
    assert A.scan_fit_plan(150, 300000, 2, -2, -5, -2, min_score=-5000) == (1024, 464, 293, 292)
    assert A.scan_fit_plan(150, 300000, 2, -2, -5, -2, tile_cols=2048) == (2048, 464, 147, 146)
    assert A.scan_fit_plan(150, 2048 * 3, 2, -2, -5, -2, tile_cols=2048)[2:] == (3, 3)
    # 20 rows: lb = -47, g = floor(87 / 2) = 43, ov = 64
    assert A.scan_fit_plan(20, 100, 2, -2, -5, -2, tile_cols=16) == (16, 64, 7, 6)
    assert A.scan_fit_plan(20, 70, 2, -2, -5, -2, tile_cols=16)[2:] == (5, 0)             # a target shorter than one full tile
    assert A.scan_fit_plan(20, 20, 2, -2, -5, -2, tile_cols=16)[2:] == (2, 0)
    assert A.scan_fit_plan(20, 19, 2, -2, -5, -2, tile_cols=16)[2:] == (0, 0)             # shorter than the query: no candidate
    # 2/-6/-2/-1, 40 rows: lb = -243, g = 323, ov = round16up(364) = 368
    assert A.scan_fit_plan(40, 1000, *TRUNC, tile_cols=64) == (64, 368, 16, 15)
    for bad in (24, 8, -16, 1000):
        with pytest.raises(A.AlignToolsError) as ei:
            A.scan_fit_plan(100, 1000, 2, -2, -5, -2, tile_cols=bad)
        assert ei.value.code == A.ERR_ARG and "multiple of 16" in str(ei.value)
    for m, u, o, e, l1 in ((0, -2, -5, -2, 10), (2, -2, 0, -2, 10), (2, -2, -5, 0, 10), (2, -2, -5, -2, 1025), (2, -2, -5, -2, 0)):
        with pytest.raises(A.AlignToolsError) as ei:
            A.scan_fit_plan(l1, 1000, m, u, o, e)
        assert ei.value.code == A.ERR_DOMAIN, (m, u, o, e, l1)
    assert A.scan_fit_plan(1024, 5000, 1024, 0, -1, -1)[0] == 1024                        # no bound on m * length: the key holds any int32


def test_window_export(lib):
    # 150 rows, 2/-2/-5/-2, a perfect hit: g = 0, ceil(5 / 2) = 3: ws = (j* - 150 - 3 - 1) & ~15, we = j* + 1
    assert A.scan_fit_window(100000, 300, 150, 300000, 2, -2, -5, -2) == (99840, 100001)
    assert A.scan_fit_window(150, 300, 150, 300000, 2, -2, -5, -2) == (0, 151)
    assert A.scan_fit_window(120, 200, 150, 300000, 2, -2, -5, -2) == (0, 150)            # at least len1 columns
    assert A.scan_fit_window(299999, 280, 150, 300000, 2, -2, -5, -2) == ((299999 - 150 - 10 - 4) & ~15, 300000)
    for args, code in (((300000, 300, 150, 300000, 2, -2, -5, -2), A.ERR_ARG), ((-1, 300, 150, 300000, 2, -2, -5, -2), A.ERR_ARG),
                       ((10, 0, 150, 100, 2, -2, -5, -2), A.ERR_ARG), ((10, 0, 15, 100, 2, -2, 0, -2), A.ERR_DOMAIN),
                       ((10, 0, 1025, 3000, 2, -2, -5, -2), A.ERR_DOMAIN)):
        with pytest.raises(A.AlignToolsError) as ei:
            A.scan_fit_window(*args)
        assert ei.value.code == code, args


def test_python_side_argument_errors():
    al = object.__new__(A.Aligner)                              # no handle: both errors come before the library is asked
    al._h = None
    with pytest.raises(ValueError):
        al.scan_fit(["ACGT"], ["ACGT"], strands="sideways")
    with pytest.raises(TypeError):
        al.scan_fit(["ACGT"], ["ACGT"], cutoff=3)               # the bound is called min_score here
    import inspect
    assert str(inspect.signature(A.Aligner.scan_fit)) == \
        "(self, queries, targets, k=1, min_score=None, strands='forward', cigar=False, cigar_m=False, tile_cols=0)"
    # the existing methods are as they were
    assert str(inspect.signature(A.Aligner.scan_local)) == str(inspect.signature(A.Aligner.scan_fit))
    assert str(inspect.signature(A.Aligner.scan)) == "(self, queries, targets, k=1, cutoff=None, strands='forward', cigar=False, cigar_m=False, tile_cols=0)"


# ---------------------------------------------------------------- CPU: the facts, on the oracle

def _tiles(l1, l2, sc, min_score, tile_cols, ov_override=None):
    """[(s0, e)] of every swept tile: it sweeps the target columns (s0, e] and owns the end columns n T <= j < (n + 1) T"""
    T, ov, ntiles, nfull = A.scan_fit_plan(l1, l2, sc[0], sc[1], sc[2], sc[3], min_score, tile_cols)
    out = []
    if ov_override is not None:                                # the control: the same cut with too little in front
        for n in range(ntiles):
            s0 = max(0, n * T - ov_override)
            e = min(l2, s0 + T + ov_override)
            if e - s0 >= l1:                                   # (fit takes no pair with l1 > l2: such a tile reports nothing)
                out.append((s0, e))
        return out
    dropped = min(ntiles - 1, ov // T)                         # the tiles 1 .. dropped would repeat tile 0's sweep: not swept
    for n in range(ntiles):
        s0 = max(0, n * T - ov)
        e = min(l2, s0 + T + ov)
        if 1 <= n <= dropped:
            assert s0 == 0 and e == min(l2, T + ov) and min(l2, (n + 1) * T) <= e
            continue
        assert (e - s0 == T + ov) == (n < nfull) and e >= min(l2, (n + 1) * T) and s0 % 16 == 0 and e - s0 >= l1
        out.append((s0, e))
    return out


def _tile_merge(q, t, sc, min_score, tile_cols, ov_override=None, state_in_key=False):
    """the lexicographic minimum of (-score, state is LOW, s0 + end_j) over the tiles, each swept as an ordinary fit pair"""
    best = None
    for s0, e in _tiles(len(q), len(t), sc, min_score, tile_cols, ov_override):
        r = O.align(FIT, q, t[s0:e], sc[0], sc[1], sc[2], sc[3])
        if r["rc"] != 0:
            assert e - s0 == 1                                  # one row x one column: the end scan has no cell
            continue
        key = (-r["score"], r["state"] if state_in_key else int(r["state"] == A.ST_LOW), s0 + r["end_j"])
        best = key if best is None or key < best else best
    if best is None:
        return None
    low = best[1] == A.ST_LOW if state_in_key else best[1] == 1
    return (-best[0], A.ST_LOW if low else A.ST_MID, best[2])


def _plant(rng, t, body):
    at = rng.randint(0, max(0, len(t) - len(body)))
    t[at:at + len(body)] = body


def _fact_pairs(n_pairs, seed):
    """random pairs with l1 <= l2 over three alphabets, the six scorings and four widths, planted copies carrying substitutions
    and indels"""
    rng = random.Random(seed)
    pairs = []
    for n in range(n_pairs):
        alpha = ("ACGT", "ACGT", "AC", "A")[n % 4]
        l1 = rng.randint(1, 64)
        l2 = l1 + rng.choice((0, 1, 2, 15, 16, 17)) if n % 17 == 0 else rng.randint(max(l1, 2), 1500)
        l2 = max(l2, 2)
        q = _rnd(rng, l1, alpha)
        t = list(_rnd(rng, l2, alpha if n % 5 else "ACGT"))
        for _ in range(rng.randint(0, 3) if n % 3 else 0):
            body = list(q)
            for _ in range(rng.randint(0, 3)):
                body[rng.randrange(len(body))] = rng.choice("ACGT")
            for _ in range(rng.randint(0, 2)):
                x = rng.randrange(len(body))
                if rng.random() < 0.5 and len(body) > 4:
                    del body[x:x + rng.randint(1, 3)]
                else:
                    body[x:x] = list(_rnd(rng, rng.randint(1, 4)))
            _plant(rng, t, body)
        pairs.append((q, "".join(t)[:l2], CPU_SCORINGS[n % 6], (16, 32, 64, 256)[(n // 6) % 4]))
    return pairs


def _trunc_pairs(n_pairs, seed):
    """2/-6/-2/-1 with copies that lack the read's last 1 to 3 bases, followed by bases the read does not continue with"""
    rng = random.Random(seed)
    pairs = []
    for n in range(n_pairs):
        l1 = rng.randint(8, 64)
        l2 = rng.randint(l1 + 8, 1200)
        q = _rnd(rng, l1)
        t = list(_rnd(rng, l2))
        for _ in range(rng.randint(1, 2)):
            cut = rng.randint(1, 3)
            body = list(q[:-cut]) + ["ACGT"[("ACGT".index(c) + 1 + rng.randrange(3)) % 4] for c in q[-cut:]]
            if n % 4 == 0:
                body[rng.randrange(len(body) - cut)] = rng.choice("ACGT")
            _plant(rng, t, body)
        pairs.append((q, "".join(t), TRUNC, (16, 32, 64, 256)[n % 4]))
    return pairs


def _edge_pairs():
    rng = random.Random(77)
    out = []
    for l1, T, sc in ((1, 16, SCORINGS[0]), (7, 16, SCORINGS[1]), (16, 16, TRUNC), (30, 32, SCORINGS[2]), (64, 64, CPU_SCORINGS[3])):
        q = _rnd(rng, l1)
        for l2 in sorted({max(l1, 2), l1 + 1, max(T, l1), max(T + 1, l1), 4 * T, 4 * T + 1}):
            t = list(_rnd(rng, l2))
            out.append((q, "".join(t), sc, T))
            t[l2 - l1:] = q                                     # the copy ends in the target's last column: the end scan leaves it out
            out.append((q, "".join(t), sc, T))
            if l2 > l1:
                t = list(_rnd(rng, l2))
                t[l2 - 1 - l1:l2 - 1] = q                       # ... and in the last column it takes
                out.append((q, "".join(t), sc, T))
    out += [("A" * l1, "CGT" * l2, sc, T) for l1, l2, sc, T in ((1, 1, SCORINGS[0], 16), (7, 200, SCORINGS[1], 16), (64, 400, SCORINGS[2], 32),
                                                                (30, 333, TRUNC, 64), (5, 90, CPU_SCORINGS[4], 256))]
    return out


_FACTS = {}


def _facts():
    """the pairs of the fact tests with the oracle's result on the whole target, computed once"""
    if not _FACTS:
        for name, pairs in (("mixed", _fact_pairs(420, 2018)), ("trunc", _trunc_pairs(160, 2019)), ("edges", _edge_pairs()),
                            ("cutoff", _fact_pairs(330, 2020) + _trunc_pairs(150, 2021))):
            _FACTS[name] = [(q, t, sc, T, _fit(q, t, sc)) for q, t, sc, T in pairs]
    return _FACTS


def test_tile_fact():
    f = _facts()
    assert len(f["mixed"]) >= 400 and len(f["trunc"]) >= 150
    low = negative = 0
    for q, t, sc, T, r in f["mixed"] + f["trunc"] + f["edges"]:
        assert _tile_merge(q, t, sc, None, T) == _hit(r), (q, t, sc, T)
        low += r["state"] == A.ST_LOW
        negative += r["score"] < 0
        assert r["end_i"] == len(q) and 1 <= r["end_j"] <= len(t) - 1
    assert low >= 20 and negative >= 20, (low, negative)        # hits in state LOW and negative scores do occur
    assert sum(r["state"] == A.ST_LOW for *_x, r in f["trunc"]) >= 20
    assert sum(r["end_j"] == len(t) - 1 for _q, t, _sc, _T, r in f["edges"]) >= 5
    # the key needs a bit of its own that says LOW: with the state's value in its place (LOW = 1 < MID = 2) an L end wins a tie it loses
    assert A.ST_LOW < A.ST_MID
    assert sum(_tile_merge(q, t, sc, None, T, state_in_key=True) != _hit(r) for q, t, sc, T, r in f["trunc"]) >= 1


def test_tile_fact_with_a_cutoff():
    under = exact = 0
    for n, (q, t, sc, T, r) in enumerate(_facts()["cutoff"]):
        top, lb = max(sc[0], sc[1]) * len(q), min(sc[0], sc[1]) * len(q) + sc[2] + sc[3]
        cutoff = lb + ((top - lb) * (1 + n % 4)) // 4 - (n % 3)
        got = _tile_merge(q, t, sc, cutoff, T)
        if r["score"] >= cutoff:
            exact += 1
            assert got == _hit(r), (q, t, sc, T, cutoff)
        else:
            under += 1
            assert got is None or (got[0] < cutoff and got[0] <= r["score"]), (q, t, sc, T, cutoff, got)   # no false hit
    assert under >= 40 and exact >= 40, (under, exact)


def test_window_fact():
    f = _facts()
    cut = low = 0
    for q, t, sc, _T, r in f["mixed"][:240] + f["trunc"][:80] + f["edges"]:
        ws, we = A.scan_fit_window(r["end_j"], r["score"], len(q), len(t), *sc)
        assert ws % 16 == 0 and 0 <= ws <= r["end_j"] < we <= len(t) and we - ws >= len(q)
        cut += ws > 0
        low += r["state"] == A.ST_LOW
        w = _fit(q, t[ws:we], sc)
        assert (w["score"], w["end_i"], w["end_j"], w["state"]) == (r["score"], r["end_i"], r["end_j"] - ws, r["state"]), (q, t, sc)
        assert w["ops"] == r["ops"], (q, t, sc)
    assert cut >= 60 and low >= 20, (cut, low)                  # the windows do cut targets


def test_control_overlap_of_16_goes_wrong():
    wrong = 0
    for q, t, sc, T, r in _facts()["mixed"][:240]:
        wrong += _tile_merge(q, t, sc, None, T, ov_override=16) != _hit(r)
    assert wrong >= 10, wrong                                   # the inputs do discriminate


# ---------------------------------------------------------------- GPU

# both sides of the tops of the 4-, 8- and 16-lane families and of fit's one-strip classes (32 lanes x 13 rows; csrc/at_classes.h), plus 1
# and 1 024; test_both_sides_of_every_row_class_edge has the edges between the classes of a family
QLENS = (1, 76, 77, 152, 153, 304, 305, 416, 417, 1024)


@pytest.fixture(scope="module")
def al():
    a = A.Aligner(0)
    yield a
    a.close()


def _mutate(rng, s, nsub, ndel, nins):
    b = list(s)
    for _ in range(nsub):
        x = rng.randrange(len(b))
        b[x] = "ACGT"[("ACGT".index(b[x]) + 1 + rng.randrange(3)) % 4]
    for _ in range(ndel):
        x = rng.randrange(1, len(b) - 3)
        del b[x:x + rng.randint(1, 3)]
    for _ in range(nins):
        x = rng.randrange(1, len(b) - 1)
        b[x:x] = list(_rnd(rng, rng.randint(1, 3)))
    return "".join(b)


def _put(t, q, end):
    assert end - len(q) >= 0 and end <= len(t)
    t[end - len(q):end] = q


@pytest.fixture(scope="module")
def sets():
    """queries at the class edges; targets of 1 500 to 3 000 bases with copies planted as given, reverse-complemented, with
    substitutions, indels and cut-off ends: ending on an own-range start of every width (a multiple of 1 024: the last column the tile
    in front sweeps), one column before and after it, in the last column the end scan takes (l2 - 1) and in the one it leaves out
    (l2), the same copy twice in one target and in two targets; a target shorter than most queries"""
    rng = random.Random(1818)
    queries = [_rnd(rng, n) for n in QLENS]
    a, b, c = list(_rnd(rng, 3000)), list(_rnd(rng, 1501)), list(_rnd(rng, 2600))
    _put(a, queries[1], 76)                                     # starts in column 1
    _put(a, queries[3], 1024); _put(a, queries[4], 1023 - 152); _put(a, _rc(queries[2]), 1025 + 153 + 77)
    _put(a, _mutate(rng, queries[5], 6, 1, 1), 2048); _put(a, queries[6], 2999)          # ends in column l2 - 1
    _put(b, queries[2], 128); _put(b, _rc(_mutate(rng, queries[7], 9, 2, 1)), 700)
    _put(b, _mutate(rng, queries[8], 3, 1, 0)[:-2], 1200); _put(b, queries[3], 1501)     # ends in column l2: not a full-score hit
    for end in (500, 1024 + 153 + 40, 2600 - 10):                # the same exact copy in several tiles: the tie goes to the first
        _put(c, queries[4], end)
    _put(c, _mutate(rng, queries[9], 30, 3, 2), 1100 + 1024)
    _put(c, queries[7][:-3], 2048 - 3 + 0)                      # a copy without its last three bases
    targets = ["".join(a), "".join(b), "".join(c), _rnd(rng, 100), "".join(a), "A" * 1600]
    queries.append("A" * 70)                                    # poly-A in poly-A
    return queries, targets


@pytest.fixture(scope="module")
def sets_n():
    """an 8-bit set: reads and targets with N"""
    rng = random.Random(88)
    queries = [_rnd(rng, 40) + "N" * 5 + _rnd(rng, 20), _rnd(rng, 153), "ACGT" * 10 + "N" * 3]
    n_run = "N" * 300 + queries[1] + "N" * 500 + _mutate(rng, queries[0], 3, 0, 1) + "N" * 200 + _rnd(rng, 600)
    return queries, [n_run, _rnd(rng, 50), _rnd(rng, 900) + queries[2] + "NNNN"]


def _brute(queries, targets, sc, strands=(0, 1)):
    """the oracle on every candidate (query, strand, whole target); a target shorter than the query is no candidate: score None"""
    nq, nt = len(queries), len(targets)
    seqs = [queries, [_rc(q) for q in queries]]
    full = {name: np.zeros((nq, 2, nt), dtype=np.int64) for name in ("score", "end_i", "end_j", "state")}
    full["cand"] = np.zeros((nq, 2, nt), dtype=bool)
    ops = {}
    for q in range(nq):
        for s in strands:
            for t in range(nt):
                if len(targets[t]) < len(queries[q]):
                    continue
                r = _fit(seqs[s][q], targets[t], sc)
                full["cand"][q, s, t] = True
                for name in ("score", "end_i", "end_j", "state"):
                    full[name][q, s, t] = r[name]
                ops[q, s, t] = r["ops"]
    return full, ops


_BRUTE = {}


def _brute_of(sets, sc, strands=(0, 1)):
    key = (id(sets), sc, strands)
    if key not in _BRUTE:
        _BRUTE[key] = _brute(sets[0], sets[1], sc, strands)
    return _BRUTE[key]


def _expected(full, strands, k, min_score):
    nq, _, nt = full["score"].shape
    out = {name: np.full((nq, k), -1 if name in ("target", "strand") else 0, dtype=np.int64)
           for name in ("target", "score", "end_i", "end_j", "state", "strand")}
    nhits = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        # candidates in (target, strand) order, so that a stable sort by score leaves ties in the rule's order
        cand = [(t, s) for t in range(nt) for s in strands if full["cand"][q, s, t]]
        if min_score is not None:
            cand = [(t, s) for t, s in cand if full["score"][q, s, t] >= min_score]
        cand.sort(key=lambda ts: -full["score"][q, ts[1], ts[0]])
        cand = cand[:k]
        nhits[q] = len(cand)
        for e, (t, s) in enumerate(cand):
            out["target"][q, e], out["strand"][q, e] = t, s
            for name in ("score", "end_i", "end_j", "state"):
                out[name][q, e] = full[name][q, s, t]
    out["nhits"] = nhits
    return out


def _same(got, want, names, what):
    for name in names:
        assert np.array_equal(np.asarray(got[name], dtype=np.int64), np.asarray(want[name], dtype=np.int64)), (what, name, got[name], want[name])


def _check_cigars(got, queries, targets, full_ops, merge):
    full, ops = full_ops
    nq, k = got["target"].shape
    for q in range(nq):
        for e in range(k):
            t = int(got["target"][q, e])
            if t < 0:
                assert int(got["ncigar"][q, e]) == 0 and (got["stats"][q, e] == -1).all() and len(got["cigar"][q][e]) == 0
                continue
            s = int(got["strand"][q, e]) if "strand" in got else 0
            s1 = queries[q] if s == 0 else _rc(queries[q])
            words, stats = A.cigar(ops[q, s, t], s1, int(full["end_i"][q, s, t]), targets[t], int(full["end_j"][q, s, t]), extended=not merge)
            assert int(got["ncigar"][q, e]) == len(words), (q, e)
            assert np.array_equal(got["cigar"][q][e], words), (q, e)
            assert np.array_equal(got["stats"][q, e], stats), (q, e, got["stats"][q, e], stats)


@pytest.mark.gpu
@pytest.mark.parametrize("tile_cols", [16, 64, 0])
@pytest.mark.parametrize("sc", SCORINGS, ids=["2-2-5-2", "1-2-5-1", "5-4-10-1", "2-6-2-1"])
def test_lists_equal_the_oracle_on_the_whole_target(al, sets, sc, tile_cols):
    queries, targets = sets
    first = sc == SCORINGS[0]
    strands = "both" if first else "forward"
    full_ops = _brute_of(sets, sc, (0, 1) if first else (0,))
    al.set_scoring(sc[0], sc[1], sc[2], sc[3])
    for k in ((1, 3, 64) if first or tile_cols == 64 else (3,)):
        cg = k == 3
        got = al.scan_fit(queries, targets, k=k, strands=strands, tile_cols=tile_cols, cigar=cg, cigar_m=cg and tile_cols == 64)
        cfg = al.last_config
        assert cfg.startswith("scan-fit: tile=%d overlap=" % (tile_cols or 1024)) and " tiles=" in cfg and " slices, k=%d; " % k in cfg and " sweep=" in cfg, cfg
        _same(got, _expected(full_ops[0], STRANDS_OF[strands], k, None), NAMES + (("strand",) if strands == "both" else ()), (sc, tile_cols, k))
        if cg:
            assert "; windows: " in cfg, cfg
            _check_cigars(got, queries, targets, full_ops, tile_cols == 64)


# the last read length of every row class of the 4-, 8-, 16- and 32-lane families up to fit's longest one-strip class (csrc/at_classes.h)
CLASS_TOPS = (36, 40, 48, 52, 56, 64, 76, 80, 96, 104, 112, 128, 152, 160, 208, 224, 256, 304, 320, 384, 416)


@pytest.mark.gpu
def test_both_sides_of_every_row_class_edge(al):
    """a read of each class's last length and one base more, each planted once with a substitution and a deletion, against two targets"""
    rng = random.Random(416)
    queries = [_rnd(rng, n + d) for n in CLASS_TOPS for d in (0, 1)]
    t = [list(_rnd(rng, 2400)), list(_rnd(rng, 1700))]
    for x, q in enumerate(queries):
        body = _mutate(rng, q, 1, 1, 0) if len(q) > 40 else q
        _put(t[x % 2], body, rng.randint(len(body), len(t[x % 2]) - 1))
    targets = ["".join(t[0]), "".join(t[1])]
    sc = SCORINGS[0]
    full_ops = _brute(queries, targets, sc, (0,))
    al.set_scoring(*sc)
    for tile_cols in (64, 0):
        got = al.scan_fit(queries, targets, k=2, tile_cols=tile_cols, cigar=True)
        assert " %d blocks, " % len(queries) in al.last_config, al.last_config      # every length is a block of its own
        _same(got, _expected(full_ops[0], (0,), 2, None), NAMES, tile_cols)
        _check_cigars(got, queries, targets, full_ops, False)


@pytest.mark.gpu
def test_eight_bit_words(al, sets_n):
    queries, targets = sets_n
    sc = SCORINGS[0]
    full_ops = _brute(queries, targets, sc)
    al.set_scoring(*sc)
    for tile_cols in (64, 0):
        got = al.scan_fit(queries, targets, k=3, strands="both", tile_cols=tile_cols, cigar=True)
        assert "bits=8" in al.last_config, al.last_config
        _same(got, _expected(full_ops[0], (0, 1), 3, None), NAMES + ("strand",), tile_cols)
        _check_cigars(got, queries, targets, full_ops, False)


@pytest.mark.gpu
def test_placements_and_ties(al, sets):
    queries, targets = sets
    sc = SCORINGS[0]
    full, _ops = _brute_of(sets, sc)
    # the planted copies are where the fixture put them (exact copies score 2 * length)
    for q, t, end in ((1, 0, 76), (3, 0, 1024), (4, 0, 1023 - 152), (6, 0, 2999), (2, 1, 128), (4, 2, 500)):
        assert (full["score"][q, 0, t], full["end_i"][q, 0, t], full["end_j"][q, 0, t], full["state"][q, 0, t]) == (2 * QLENS[q], QLENS[q], end, A.ST_MID), (q, t)
    assert full["score"][2, 1, 0] == 2 * 77 and full["end_j"][2, 1, 0] == 1025 + 153 + 77
    assert len(targets[1]) - 1 == 1500 and full["score"][3, 0, 1] < 2 * 152        # the copy that ends in column l2 is not taken whole
    assert len(targets[0]) - 1 == 2999                                            # ... the one that ends in l2 - 1 is
    assert (full["score"][10, 0, 5], full["end_j"][10, 0, 5]) == (140, 70)        # poly-A: the first column that has it
    short = [q for q in range(len(queries)) if len(queries[q]) > len(targets[3])]
    assert len(short) >= 7 and not full["cand"][short, :, 3].any()                # reads longer than a target
    al.set_scoring(*sc)
    for tile_cols in (16, 64, 0):
        got = al.scan_fit(queries, targets, k=6, strands="both", tile_cols=tile_cols)
        _same(got, _expected(full, (0, 1), 6, None), NAMES + ("strand",), tile_cols)
        assert list(got["target"][3, :2]) == [0, 4] and list(got["end_j"][3, :2]) == [1024, 1024]   # equal scores: the smaller index first
        assert (got["target"][4, :3] == [0, 2, 4]).all() and int(got["end_j"][4, 1]) == 500      # three times in one target: the smallest j
        assert int(got["nhits"][9]) == 6 and 3 not in got["target"][9]            # the short target is no candidate, and no error


def _tie_case():
    """2/-6/-2/-1, a read of 40 bases: an early copy without its last base (then bases the read does not end in): 2 * 39 - 2 = 76 in
    state LOW; a later copy that lacks one base in the middle: 2 * 39 - 2 = 76 in state MID.  M before L at equal score"""
    rng = random.Random(4040)
    q = _rnd(rng, 38) + "AC"                                    # (the last two bases differ: the closing gap row has one place)
    other = "ACGT"[("ACGT".index(q[-1]) + 1) % 4]
    low_copy = q[:-1] + other * 4
    mid_copy = q[:20] + q[21:]
    t = list(_rnd(rng, 1500))
    _put(t, low_copy, 303)
    _put(t, mid_copy, 1100)
    t = "".join(t)
    a, b, r = _fit(q, t[:600], TRUNC), _fit(q, t[600:], TRUNC), _fit(q, t, TRUNC)
    assert (a["score"], a["state"], a["end_j"]) == (76, A.ST_LOW, 299) and (b["score"], b["state"], b["end_j"] + 600) == (76, A.ST_MID, 1100)
    assert _hit(r) == (76, A.ST_MID, 1100)
    return q, t, r


def test_tie_case_on_the_oracle():
    q, t, r = _tie_case()
    for T in (16, 64, 256):
        assert _tile_merge(q, t, TRUNC, None, T) == _hit(r)
        assert _tile_merge(q, t, TRUNC, None, T, state_in_key=True) == (76, A.ST_LOW, 299)    # the key without a LOW bit goes wrong here


@pytest.mark.gpu
def test_m_end_before_l_end_at_equal_score(al):
    q, t, r = _tie_case()
    al.set_scoring(*TRUNC)
    for tile_cols in (16, 64, 0):
        got = al.scan_fit([q], [t, t[:600]], k=2, tile_cols=tile_cols, cigar=True)
        assert (list(got["score"][0]), list(got["state"][0]), list(got["end_j"][0]), list(got["target"][0])) == ([76, 76], [A.ST_MID, A.ST_LOW], [1100, 299], [0, 1])
        words, stats = A.cigar(r["ops"], q, 40, t, 1100)
        assert np.array_equal(got["cigar"][0][0], words) and np.array_equal(got["stats"][0, 0], stats)
        assert A.cigar_string(got["cigar"][0][1]) == b"39=1I", A.cigar_string(got["cigar"][0][1])


@pytest.mark.gpu
def test_end_columns_at_tile_borders(al):
    """exact copies that end in the last column a tile sweeps (a multiple of the width: the next tile owns it), one column before and
    after it, and in l2 - 1"""
    rng = random.Random(5)
    reads = [_rnd(rng, n) for n in (20, 77, 153)]
    for T, l2 in ((64, 1500), (0, 3000)):
        w = T or 1024
        ends = [w, 3 * w - 1, 3 * w + 1 + 153] if T else [1024, 2047, 2049 + 153]
        t = list(_rnd(rng, l2))
        for r, end in zip(reads, ends):
            _put(t, r, end)
        last = list(_rnd(rng, l2))
        _put(last, reads[1], l2 - 1)
        al.set_scoring(*SCORINGS[0])
        got = al.scan_fit(reads, ["".join(t), "".join(last)], k=2, tile_cols=T, cigar=True)
        assert list(got["end_j"][:, 0]) == ends and list(got["target"][:, 0]) == [0, 0, 0], (T, got["end_j"], got["target"])
        assert list(got["score"][:, 0]) == [40, 154, 306] and (got["state"] == A.ST_MID).all()
        assert (int(got["target"][1, 1]), int(got["score"][1, 1]), int(got["end_j"][1, 1])) == (1, 154, l2 - 1)   # the last column the end scan takes
        assert [A.cigar_string(x[0]) for x in got["cigar"]] == [b"20=", b"77=", b"153="] and A.cigar_string(got["cigar"][1][1]) == b"77="
        assert list(got["stats"][:, 0, 1]) == [e - n for e, n in zip(ends, (20, 77, 153))] and int(got["stats"][1, 1, 1]) == l2 - 1 - 77


@pytest.mark.gpu
@pytest.mark.parametrize("strands", ["forward", "reverse", "both"])
def test_equals_search_fit(al, sets, strands):
    queries, targets = sets
    al.set_scoring(*SCORINGS[0])
    for k, min_score in ((1, None), (5, None), (64, 60)):
        want = al.search("fit", queries, targets, k=k, cutoff=min_score, strands=strands)
        for tile_cols in (64, 0):
            got = al.scan_fit(queries, targets, k=k, min_score=min_score, strands=strands, tile_cols=tile_cols)
            _same(got, want, NAMES + (("strand",) if strands != "forward" else ()), (strands, k, min_score, tile_cols))


def _slice_sets():
    rng = random.Random(3)
    queries = [_rnd(rng, n) for n in (20, 39, 77, 20, 257)]
    body = list(_rnd(rng, 700))
    body[100:120] = queries[0]; body[340:379] = queries[1]; body[600:677] = _rc(queries[2])
    wide = list(_rnd(rng, 2600))
    wide[900:1157] = queries[4]                                # across the first own-range end of the default width
    return queries, ["".join(body), _rnd(rng, 90), queries[3] + _rnd(rng, 200), "".join(wide)]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, None])
def test_slices_give_identical_lists(al, monkeypatch, chunk):
    """AT_ALLPAIRS_CHUNK = 1: one tile pair per slice, a pair's slot lives through all of them"""
    queries, targets = _slice_sets()
    sc = SCORINGS[0]
    key = ("slices", sc)
    if key not in _BRUTE:
        _BRUTE[key] = _brute(queries, targets, sc)
    full_ops = _BRUTE[key]
    if chunk is None:
        monkeypatch.delenv("AT_ALLPAIRS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("AT_ALLPAIRS_CHUNK", str(chunk))
    al.set_scoring(*sc)
    got = al.scan_fit(queries, targets, k=3, strands="both", tile_cols=256, cigar=True)
    if chunk is not None:
        cfg = al.last_config
        tiles, slices = int(cfg.split("tiles=")[1].split()[0]), int(cfg.split(" blocks, ")[1].split()[0])
        assert tiles > 50 and (slices == tiles if chunk == 1 else slices >= -(-tiles // 7)), cfg
    _same(got, _expected(full_ops[0], (0, 1), 3, None), NAMES + ("strand",), chunk)
    _check_cigars(got, queries, targets, full_ops, False)
    # the default width: full-shape tiles and the shorter ones behind them
    got = al.scan_fit(queries, targets, k=3, strands="both", cigar=True)
    _same(got, _expected(full_ops[0], (0, 1), 3, None), NAMES + ("strand",), (chunk, "default width"))
    _check_cigars(got, queries, targets, full_ops, False)


@pytest.mark.gpu
def test_cigar_pieces_and_layout(al, sets, monkeypatch):
    """the window pass in pieces of 1, 5 and all hits (a piece has no more hits than a slice has pairs): the same words at the same
    offsets; unused entries take no room"""
    queries, targets = sets
    sc = SCORINGS[0]
    full_ops = _brute_of(sets, sc)
    al.set_scoring(*sc)
    ref = None
    for piece in (None, 1, 5):
        if piece is None:
            monkeypatch.delenv("AT_ALLPAIRS_CHUNK", raising=False)
        else:
            monkeypatch.setenv("AT_ALLPAIRS_CHUNK", str(piece))
        got = al.scan_fit(queries[:6], targets[:3], k=4, min_score=40, strands="both", cigar=True, tile_cols=256)
        if piece is not None:
            assert " %d pieces, " % -(-int(got["nhits"].sum()) // piece) in al.last_config, al.last_config
        n = got["target"].size
        assert 0 < int(got["nhits"].sum()) < n                  # used and unused entries
        off, nc = got["cigar_off"], got["ncigar"].reshape(-1)
        assert off[0] == 0 and np.array_equal(off[1:] - off[:-1], nc) and (nc[got["target"].reshape(-1) < 0] == 0).all()
        sub = {name: full_ops[0][name][:6, :, :3] for name in full_ops[0]}
        _same(got, _expected(sub, (0, 1), 4, 40), NAMES + ("strand",), piece)
        _check_cigars(got, queries[:6], targets, full_ops, False)
        if ref is None:
            ref = got
        for name in ("ncigar", "stats", "cigar_off"):
            assert np.array_equal(ref[name], got[name]), (piece, name)


@pytest.mark.gpu
def test_min_score_removes_hits(al, sets):
    queries, targets = sets
    sc = SCORINGS[0]
    full, _ops = _brute_of(sets, sc)
    al.set_scoring(*sc)
    for min_score in (-5, 30, 120, 400):
        want = _expected(full, (0, 1), 4, min_score)
        assert 0 < want["nhits"].sum() < 4 * len(queries)
        for tile_cols in (64, 0):
            got = al.scan_fit(queries, targets, k=4, min_score=min_score, strands="both", tile_cols=tile_cols)
            _same(got, want, NAMES + ("strand",), (min_score, tile_cols))


@pytest.mark.gpu
def test_handle_settings_neither_matter_nor_change(al, sets):
    queries, targets = sets
    al.set_scoring(*SCORINGS[0])
    a = al.scan_fit(queries[:6], targets[:3], k=2, tile_cols=64, cigar=True)
    al.set_min_score(500)
    al.set_edit_infix(True)
    al.set_edit_traceback(True)
    try:
        b = al.scan_fit(queries[:6], targets[:3], k=2, tile_cols=64, cigar=True)
        # the settings are what they were: an edit batch behind the scan still takes the infix rule (0 edits inside the target, 4 across it)
        al.set_scoring(1, 1, -1, -1)
        assert int(al.align_batch("edit", [("ACGT", "TTACGTTT")], traceback=False, render=False)["score"][0]) == 0
    finally:
        al.set_min_score(None)
        al.set_edit_infix(False)
        al.set_edit_traceback(False)
    for name in NAMES + ("ncigar", "stats", "cigar_off"):
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
def test_jump_sites_are_refused(sets):
    queries, targets = sets
    other = A.Aligner(0)
    try:
        other.set_scoring(2, -2, -5, -2, -10, True, [5, 9])
        with pytest.raises(A.AlignToolsError) as ei:
            other.scan_fit(queries[:2], targets[:1])
        assert ei.value.code == A.ERR_DOMAIN and "use_jump is set" in str(ei.value), ei.value
        other.set_scoring(2, -2, -5, -2)
        got = other.scan_fit(queries[1:2], targets[:1])
        assert (int(got["score"][0, 0]), int(got["end_j"][0, 0])) == (152, 76)
    finally:
        other.close()


@pytest.mark.gpu
def test_edges_and_refusals(al, sets):
    queries, targets = sets
    q, t = queries[:4], targets[:2]
    al.set_scoring(*SCORINGS[0])
    got = al.scan_fit([], t, k=2)
    assert got["target"].shape == (0, 2)
    got = al.scan_fit(q, [], k=2, cigar=True)
    assert (got["nhits"] == 0).all() and (got["target"] == -1).all() and (got["ncigar"] == 0).all() and (got["stats"] == -1).all()
    got = al.scan_fit(q[1:], ["ACGT", ""], k=2, cigar=True)     # every target is shorter than every query: no candidate, no error
    assert (got["nhits"] == 0).all() and (got["target"] == -1).all() and (got["ncigar"] == 0).all()
    for k in (0, 65):
        with pytest.raises(A.AlignToolsError) as ei:
            al.scan_fit(q, t, k=k)
        assert ei.value.code == A.ERR_ARG and "at_scan_fit: k = %d outside 1..64" % k in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_fit(q, t, tile_cols=24)
    assert ei.value.code == A.ERR_ARG and "at_scan_fit: tile_cols = 24 is not a positive multiple of 16 (or 0 for the default, 1024)" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_fit(q + ["ACGTA" * 205], t)
    assert ei.value.code == A.ERR_DOMAIN and "at_scan_fit: query 4 has 1025 bases: at most 1024" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_fit(q + [""], t)
    assert ei.value.code == A.ERR_DOMAIN and "query 4: empty" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_fit(["A"], ["C"])                               # one row x one column: fit's end scan has no cell
    assert ei.value.code == A.ERR_DOMAIN and "at_scan_fit: a pair outside the domain" in str(ei.value), ei.value
    for m, u, o, e in ((2, -2, -5, 0), (0, -2, -5, -2), (2, -2, 0, -2)):
        other = A.Aligner(0)
        try:
            other.set_scoring(m, u, o, e)
            with pytest.raises(A.AlignToolsError) as ei:
                other.scan_fit(q, t)
            assert ei.value.code == A.ERR_DOMAIN and "at_scan_fit needs m >= 1, o <= -1 and e <= -1" in str(ei.value), ei.value
        finally:
            other.close()
    # a tile is a pair of the batch entry: its exact-score bound is said up front with the tile's numbers
    other = A.Aligner(0)
    try:
        other.set_scoring(4200, -1, -1, -1)
        with pytest.raises(A.AlignToolsError) as ei:
            other.scan_fit([queries[9]], targets[:1])          # 4 200 * (1 024 + 3 000 + 2) >= 2^24
        assert ei.value.code == -3 and "at_scan_fit: a tile of 1024 rows x 3000 columns" in str(ei.value) and "exact score range" in str(ei.value), ei.value
        got = other.scan_fit([queries[1]], [targets[1]])        # 76 x 1 501: inside the bound
        r = _fit(queries[1], targets[1], (4200, -1, -1, -1))
        assert (int(got["score"][0, 0]), int(got["end_i"][0, 0]), int(got["end_j"][0, 0]), int(got["state"][0, 0])) == (r["score"], r["end_i"], r["end_j"], r["state"])
    finally:
        other.close()
    # the handle works afterwards
    full, _ops = _brute_of(sets, SCORINGS[0])
    got = al.scan_fit(queries, targets, k=2, tile_cols=64)
    _same(got, _expected(full, (0,), 2, None), NAMES, "after the refusals")


@pytest.mark.gpu
def test_multi_process_handle_is_refused(tmp_path):
    """a handle that has joined a multi-process job (a world of one needs no collective library): one GPU only"""
    import ctypes as C
    lib = A.load_library()
    other = A.Aligner(0)
    try:
        other.set_scoring(*SCORINGS[0])
        lib.at_comm_init.restype = C.c_int
        lib.at_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
        assert lib.at_comm_init(other._h, 0, 1, str(tmp_path).encode()) == 0, lib.at_last_error(other._h)
        with pytest.raises(A.AlignToolsError) as ei:
            other.scan_fit(["ACGT"], ["ACGTACGT"])
        assert ei.value.code == A.ERR_DOMAIN and "at_scan_fit: one GPU only" in str(ei.value), ei.value
    finally:
        other.close()


@pytest.mark.gpu
def test_eight_reads_in_300k(al):
    """every hit against the oracle on a window the test cuts itself: 600 columns that end 100 behind the planted copy"""
    rng = random.Random(300000)
    body = list(_rnd(rng, 300000))
    reads, ends = [], []
    for x, end in enumerate((150, 2048, 40961, 100000, 150000 + 77, 204800 + 149, 262145, 299999)):
        r = _rnd(rng, 150)
        planted = r if x % 4 != 3 else _mutate(rng, r, 4, 1, 0)
        body[end - len(planted):end] = planted
        reads.append(r if x % 2 == 0 else _rc(r))
        ends.append(end)
    target = "".join(body)
    al.set_scoring(*SCORINGS[0])
    got = al.scan_fit(reads, [target], k=1, strands="both", cigar=True)
    assert "scan-fit: tile=1024 overlap=464 tiles=%d " % (293 * 16) in al.last_config, al.last_config
    assert (got["nhits"] == 1).all() and (got["end_i"][:, 0] == 150).all() and list(got["strand"][:, 0]) == [0, 1] * 4
    for x, end in enumerate(ends):
        lo, hi = max(0, end - 500), min(300000, end + 100)
        r = _fit(reads[x] if x % 2 == 0 else _rc(reads[x]), target[lo:hi], SCORINGS[0])
        assert r["score"] >= 250                                # far above anything a random stretch of the target gives
        assert (int(got["score"][x, 0]), int(got["end_j"][x, 0]), int(got["state"][x, 0])) == (r["score"], lo + r["end_j"], r["state"]), x
        words, stats = A.cigar(r["ops"], reads[x] if x % 2 == 0 else _rc(reads[x]), 150, target[lo:hi], r["end_j"])
        stats[1] += lo                                          # AT_CG_START_J is absolute
        assert np.array_equal(got["cigar"][x][0], words) and np.array_equal(got["stats"][x, 0], stats), x
    assert list(got["end_j"][:, 0]) == ends
