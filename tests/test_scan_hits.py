"""at_scan_hits / Aligner.scan_hits: every occurrence of a read under a distance cutoff.

Every expected value comes from a numpy brute force on the FULL table (_table of tests/test_edit_infix.py), written from the rule in
include/aligntools_hip.h: occurrences from the run-length form of the last row, the separation as a window minimum over the
occurrences, the ops by the three-way rule from (l1, a).  Nothing is taken from the code under test.

On the CPU: the exports and the three facts the mechanism rests on, restated in numpy with the planner's own numbers -- a tile sees
exactly the descents of its own columns, the occurrences follow from the sorted descents alone, and the window of ANY occurrence
walked from its last column gives the full table's ops."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import aligntools.c_amd as A
from test_edit_infix import _table

UNIT = (1, 1, -5, -1, -10)
STRANDS_OF = {"forward": (0,), "both": (0, 1)}


def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _rc(s):
    return A.revcomp(s).decode("latin1")


# ---------------------------------------------------------------- the brute force

def _occurrences(row, l1, max_dist):
    """[(a, v)] by the definition: the first column of every run of equal values of the last row that is at or under c, lies below
    the run in front of it and is the last run or lies below the run behind it"""
    if l1 < 1:
        return []
    c = min(max_dist, l1 - 1)
    row = np.asarray(row)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(row)) + 1))
    vals = row[starts]
    out = []
    for r in range(1, len(starts)):
        v = int(vals[r])
        if v <= c and vals[r - 1] > v and (r + 1 == len(starts) or vals[r + 1] > v):
            out.append((int(starts[r]), v))
    return out


def _separate(occ, sep):
    """the occurrences that no other occurrence within sep columns beats on (v, a)"""
    if sep <= 0 or len(occ) < 2:
        return list(occ)
    a = np.array([x[0] for x in occ], dtype=np.int64)
    key = np.array([x[1] for x in occ], dtype=np.int64) * (1 << 32) + a
    lo, hi = np.searchsorted(a, a - sep, "left"), np.searchsorted(a, a + sep, "right")
    return [occ[i] for i in range(len(occ)) if key[lo[i]:hi[i]].min() == key[i]]


def _walk(a, b, D, col):
    """ops END -> START of the three-way rule from (l1, col), and j0"""
    i, j, ops = len(a), col, bytearray()
    while i > 0:
        if j > 0 and D[i - 1, j - 1] + (a[i - 1] != b[j - 1]) == D[i, j]:
            ops.append(A.OP_MID)
            i, j = i - 1, j - 1
        elif D[i - 1, j] + 1 == D[i, j]:
            ops.append(A.OP_LOW)
            i -= 1
        else:
            ops.append(A.OP_UPP)
            j -= 1
    return bytes(ops), j


class Brute:
    """last rows of every (query, strand, target), and the ops of the occurrences at or under ops_dist (walked while the table is at hand)"""

    def __init__(self, queries, targets, ops_dist=-1):
        self.queries, self.targets = queries, targets
        self.rows, self.ops = {}, {}
        for q, s1 in enumerate(queries):
            for s in (0, 1):
                x = (_rc(s1) if s else s1).encode()
                for t, s2 in enumerate(targets):
                    a, b, D = _table(x, s2.encode(), True)
                    self.rows[q, s, t] = D[len(x)].copy()
                    for col, v in (_occurrences(D[len(x)], len(x), ops_dist) if ops_dist >= 0 else []):
                        self.ops[q, s, t, col] = _walk(a, b, D, col)

    def hits(self, max_dist, min_sep, strands):
        """per query the list of (v, target, strand, a) in the order of the header"""
        out = []
        for q, s1 in enumerate(self.queries):
            mine = []
            for t in range(len(self.targets)):
                for s in STRANDS_OF[strands]:
                    occ = _occurrences(self.rows[q, s, t], len(s1), max_dist)
                    for a, v in _separate(occ, len(s1) if min_sep == A.SCAN_SEP_READ else min_sep):
                        mine.append((v, t, s, a))
            out.append(sorted(mine))
        return out


def _flat(lists):
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    rows = [h for x in lists for h in x]
    cols = [np.array([h[k] for h in rows], dtype=np.int32) for k in range(4)]
    return off, cols[1], cols[0], cols[3], cols[2]          # hit_off, target, score, end_j, strand


def _same(got, lists, ctx):
    off, target, score, end_j, strand = _flat(lists)
    assert np.array_equal(got["hit_off"], off), (ctx, got["hit_off"][:12], off[:12])
    for name, want in (("target", target), ("score", score), ("end_j", end_j), ("strand", strand)):
        bad = np.flatnonzero(got[name] != want)
        assert len(bad) == 0, (ctx, name, bad[:5], got[name][bad[:5]], want[bad[:5]])


def _check_cigars(got, brute, merge, ctx):
    q_of = np.repeat(np.arange(len(got["hit_off"]) - 1), np.diff(got["hit_off"]))
    assert len(q_of) == len(got["target"]) == len(got["cigar"])
    for e, q in enumerate(q_of):
        t, s, col = int(got["target"][e]), int(got["strand"][e]), int(got["end_j"][e])
        s1 = _rc(brute.queries[q]) if s else brute.queries[q]
        ops, j0 = brute.ops[int(q), s, t, col]
        words, stats = A.cigar(ops, s1, len(s1), brute.targets[t], col, extended=not merge)
        assert stats[1] == j0
        assert int(got["ncigar"][e]) == len(words) and np.array_equal(got["cigar"][e], words), (ctx, e, q, t, s, col)
        assert np.array_equal(got["stats"][e], stats), (ctx, e, got["stats"][e], stats)


# ---------------------------------------------------------------- CPU: exports

@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


def test_scan_hits_symbol_exported(lib):
    assert "at_scan_hits" in A.ABI_SYMBOLS and getattr(lib, "at_scan_hits") is not None
    assert A.SCAN_SEP_READ == -1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aligntools_hip.h")).read()
    assert "#define AT_SCAN_SEP_READ (-1)" in hdr


# ---------------------------------------------------------------- CPU: the facts, on the restatement

def _fact_pairs():
    rng = random.Random(313)
    pairs = []
    for n in range(400):
        alpha = ("ACGT", "ACGT", "AC", "A")[n % 4]
        l1 = rng.randint(1, 45) if n % 13 else rng.randint(60, 90)
        l2 = rng.choice((0, 1, 15, 16, 17)) if n % 17 == 0 else rng.randint(0, 500)
        q = _rnd(rng, l1, alpha)
        t = list(_rnd(rng, l2, alpha))
        for _ in range(rng.randint(0, 3) if l2 else 0):        # planted, with a few edits
            body = list(q)
            for _ in range(rng.randint(0, 4)):
                body[rng.randrange(len(body))] = rng.choice(alpha)
            if rng.random() < 0.4 and len(body) > 1:
                del body[rng.randrange(len(body))]
            at = rng.randint(0, max(0, l2 - len(body)))
            t[at:at + len(body)] = body
            t = t[:l2]
        pairs.append((q.encode(), "".join(t).encode(), (16, 32, 64)[n % 3], rng.randint(0, 45)))
    return pairs


def _descents(row, c, first=1, base=0):
    """[(base + j, row[j])] for j >= first with row[j] <= c and row[j] < row[j - 1]"""
    row = np.asarray(row)
    j = np.flatnonzero((row[1:] <= c) & (row[1:] < row[:-1])) + 1
    return [(base + int(x), int(row[x])) for x in j if x >= first]


def test_descents_are_exact_per_tile_and_give_the_valleys(lib):
    pairs = _fact_pairs()
    nvalleys = ntiles = nshorter = 0
    for q, t, T, max_dist in pairs:
        l1, l2 = len(q), len(t)
        c = min(max_dist, l1 - 1)
        row = _table(q, t, True)[2][l1]
        S = _descents(row, c)
        # fact 1: the tiles of the planner with the cutoff c see exactly S, each in its own columns
        tile, ov, ng = A.scan_plan(l1, l2, c, T)
        assert tile == T and ov == (l1 + c + 15) // 16 * 16
        seen = []
        for n in range(64 * ng):
            s0, e = max(0, n * T - ov), min((n + 1) * T, l2)
            if e <= n * T:
                break
            ntiles += 1
            seen += _descents(_table(q, t[s0:e], True)[2][l1], c, first=n * T - s0 + 1, base=s0)
        assert seen == S, (l1, l2, T, max_dist)
        # fact 2: an element of S is an occurrence iff it is the last one or the next one is not lower
        valleys = [S[i] for i in range(len(S)) if i + 1 == len(S) or S[i + 1][1] >= S[i][1]]
        assert valleys == _occurrences(row, l1, max_dist), (l1, l2, max_dist)
        nvalleys += len(valleys)
        # ... and with S as the kernel records it: one record (last column, last value, first value) per run of descents in
        # consecutive columns of one tile; a record is an occurrence iff it is the last one or the next one's first value is not lower
        runs = []
        for col, v in S:
            if runs and runs[-1][0] == col - 1 and (col - 1) % T != 0:
                runs[-1] = (col, v, runs[-1][2])
            else:
                runs.append((col, v, v))
        assert [(r[0], r[1]) for i, r in enumerate(runs) if i + 1 == len(runs) or runs[i + 1][2] >= r[1]] == valleys
        nshorter += len(runs) < len(S)
    assert nvalleys > 1500 and ntiles > 3000 and nshorter > 150


def test_anchored_window_gives_the_full_tables_ops():
    pairs = _fact_pairs()
    n = other = 0
    for q, t, _T, max_dist in pairs[::2]:
        l1 = len(q)
        a, b, D = _table(q, t, True)
        for col, v in _occurrences(D[l1], l1, max_dist):
            ops, j0 = _walk(a, b, D, col)
            ws = max(0, (col - l1 - v)) & ~15
            wa, wb, Dw = _table(q, t[ws:col], True)
            assert Dw[l1, col - ws] == v
            assert _walk(wa, wb, Dw, col - ws) == (ops, j0 - ws), (l1, len(t), col, v)
            n += 1
            other += int(np.argmin(Dw[l1])) != col - ws       # the window's own arg-min is another column: why the end is anchored
    assert n > 800 and other > 50


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    a.set_scoring(*UNIT)
    yield a
    a.close()


QLENS = (1, 31, 32, 33, 64, 65, 160, 161, 512, 513, 1024)


def _mutated(rng, q, nsub, ndel):
    m = list(q)
    for x in rng.sample(range(len(m)), nsub):
        m[x] = "ACGT"[("ACGT".index(m[x]) + 1) % 4]
    for _ in range(ndel):
        del m[rng.randrange(1, len(m) - 1)]
    return "".join(m)


@pytest.fixture(scope="module")
def sets():
    """queries at the class edges; targets of 0, 1, 15..17, ~1 000 and ~9 000 bases.  Exact and mutated copies (substitutions, one
    deletion) end on an own-range start of every width (256 n + 1), one column before and one after it, on a group boundary
    (T = 16: 1 024 n, T = 64: 4 096), and span group boundaries"""
    rng = random.Random(1213)
    Q = [_rnd(rng, n) for n in QLENS]
    t1k, t9k = list(_rnd(rng, 1003)), list(_rnd(rng, 9001))

    def plant(t, s, end):
        assert end - len(s) >= 0 and end <= len(t)
        t[end - len(s):end] = s

    plant(t1k, Q[1], 300); plant(t1k, _rc(Q[3]), 600); plant(t1k, Q[5], 1003)
    plant(t9k, Q[1], 257); plant(t9k, Q[1], 512); plant(t9k, _mutated(rng, Q[1], 2, 0), 770); plant(t9k, Q[1], 1024); plant(t9k, Q[1], 2060)
    plant(t9k, Q[3], 1300); plant(t9k, _mutated(rng, Q[3], 0, 1), 1400); plant(t9k, Q[3], 1537)
    plant(t9k, Q[5], 2305); plant(t9k, _mutated(rng, Q[5], 3, 0), 2500); plant(t9k, Q[5], 4096)
    plant(t9k, Q[6], 2800); plant(t9k, Q[6], 3150); plant(t9k, _mutated(rng, Q[6], 4, 1), 3400)
    plant(t9k, Q[7], 3585); plant(t9k, _mutated(rng, Q[7], 0, 1), 3800)
    plant(t9k, Q[8], 4700); plant(t9k, _mutated(rng, Q[8], 5, 1), 5300)
    plant(t9k, Q[9], 5900)
    plant(t9k, Q[10], 7000); plant(t9k, _mutated(rng, Q[10], 3, 1), 8100)
    plant(t9k, _rc(Q[4]), 8200); plant(t9k, Q[2], 8300); plant(t9k, Q[2], 8400); plant(t9k, _mutated(rng, Q[2], 1, 0), 8500)
    targets = ["", _rnd(rng, 1), _rnd(rng, 15), _rnd(rng, 16), _rnd(rng, 17), "".join(t1k), "".join(t9k)]
    return Q, targets


@pytest.fixture(scope="module")
def brute(sets):
    return Brute(*sets, ops_dist=12)


@pytest.fixture(scope="module")
def expected(brute):
    memo = {}

    def get(max_dist, min_sep, strands):
        key = (max_dist, min_sep, strands)
        if key not in memo:
            memo[key] = brute.hits(*key)
        return memo[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("min_sep", [0, 5, -1])
@pytest.mark.parametrize("max_dist", [0, 12, 2000])
@pytest.mark.parametrize("tile_cols", [16, 64, 256, 0])
def test_tiles_and_classes(al, sets, brute, expected, tile_cols, max_dist, min_sep, strands):
    queries, targets = sets
    cg = max_dist <= 12
    got = al.scan_hits(queries, targets, max_dist, min_sep=min_sep, strands=strands, tile_cols=tile_cols, cigar=cg,
                       cigar_m=cg and strands == "both")
    cfg = al.last_config
    assert cfg.startswith("scan-hits: tile=%d " % (tile_cols or A.scan_plan(1, 1)[0])) and "myers-scan-hits bits=2 words/lane=" in cfg, cfg
    assert "max_dist=%d min_sep=%d " % (max_dist, min_sep) in cfg, cfg
    if tile_cols == 16:
        groups = int(cfg.split("groups=")[1].split()[0])
        assert groups == sum(max(1, -(-len(t) // 1024)) for t in targets) and groups > len(targets)      # several groups per long target
    want = expected(max_dist, min_sep, strands)
    _same(got, want, (tile_cols, max_dist, min_sep, strands))
    assert "kept=%d " % sum(len(x) for x in want) in cfg, cfg
    if max_dist == 0 and strands == "forward":
        # the planted exact copies, every one of them
        assert [h[3] for h in want[1] if h[1] == 6] == [257, 512, 1024, 2060]
        assert [h[3] for h in want[2] if h[1] == 6] == [8300, 8400]
    if cg:
        assert "windows: myers-infix-tb" in cfg, cfg
        _check_cigars(got, brute, strands == "both", (tile_cols, max_dist, min_sep, strands))


@pytest.fixture(scope="module")
def plateau_sets():
    rng = random.Random(4)
    pal = _rc(_rnd(rng, 20))
    pal = _rc(pal) + pal
    assert _rc(pal) == pal
    fall = "A" * 30 + "CGTCGT"
    queries = ["A" * 70, "ACGT" * 12, fall, pal, _rnd(rng, 300)]
    targets = ["A" * 2500, _rnd(rng, 700) + "ACGT" * 40 + _rnd(rng, 300) + "ACGT" * 12 + "ACGA" + "ACGT" * 3 + _rnd(rng, 100),
               _rnd(rng, 1000, "CGT") + "A" * 100 + "CGTCGT" + _rnd(rng, 200, "CGT"), _rnd(rng, 1500) + pal + _rnd(rng, 40) + pal, _rnd(rng, 120)]
    return queries, targets


@pytest.fixture(scope="module")
def plateau_brute(plateau_sets):
    return Brute(*plateau_sets, ops_dist=8)


@pytest.mark.gpu
@pytest.mark.parametrize("min_sep", [0, 3, -1])
def test_plateaus_and_descents(al, plateau_sets, plateau_brute, min_sep):
    queries, targets = plateau_sets
    b = plateau_brute
    # what the cases are about, on the brute force itself
    assert _occurrences(b.rows[0, 0, 0], 70, 8) == [(70, 0)]                                   # poly-A in poly-A: one hit, one candidate
    assert len(_descents(b.rows[0, 0, 0], 0)) == 1
    tandem = [a for a, v in _occurrences(b.rows[1, 0, 1], 48, 0)]
    assert tandem[:29] == list(range(748, 861, 4))                                             # a valley every 4 columns
    row = b.rows[2, 0, 2]
    assert row[1029] == 7 and (row[1030:1101] == 6).all() and list(row[1101:1107]) == [5, 4, 3, 2, 1, 0]
    assert (1030, 6) in _descents(row, 8) and [x for x in _occurrences(row, 36, 8) if 1000 < x[0] < 1110] == [(1106, 0)]
    assert len(queries[4]) > len(targets[4])                                                   # a read longer than its target
    for strands in ("forward", "both"):
        for max_dist in (0, 8):
            got = al.scan_hits(queries, targets, max_dist, min_sep=min_sep, strands=strands, tile_cols=16, cigar=True)
            want = b.hits(max_dist, min_sep, strands)
            _same(got, want, (min_sep, strands, max_dist))
            _check_cigars(got, b, False, (min_sep, strands, max_dist))
            if max_dist == 8:
                mine = [(h[3], h[0]) for h in want[2] if h[1] == 2 and h[2] == 0]
                assert (1106, 0) in mine and not any(1030 <= a < 1106 for a, _v in mine)       # the plateau that falls on is no hit
            if strands == "both" and min_sep == 0:
                both = [(h[2], h[3]) for h in want[3] if h[1] == 3 and h[0] == 0]
                assert both == [(0, 1540), (0, 1620), (1, 1540), (1, 1620)]                    # its own reverse complement: strand 0 first


@pytest.mark.gpu
def test_a_window_with_a_better_column(al, plateau_sets, plateau_brute):
    """hits whose window holds a lower or an earlier equal column than its last one: the case that needs the anchored end"""
    queries, targets = plateau_sets
    want = plateau_brute.hits(8, 0, "forward")
    lower = earlier = 0
    for q, mine in enumerate(want):
        for v, t, _s, a in mine:
            l1 = len(queries[q])
            ws = max(0, a - l1 - v) & ~15
            roww = _table(queries[q].encode(), targets[t][ws:a].encode(), True)[2][l1]
            assert roww[a - ws] == v
            lower += int(roww.min()) < v
            earlier += int(np.argmin(roww)) < a - ws
    assert lower >= 1 and earlier > lower
    got = al.scan_hits(queries, targets, 8, min_sep=0, cigar=True, tile_cols=64)
    _same(got, want, "windows")
    _check_cigars(got, plateau_brute, False, "windows")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, None])
def test_slices_and_capacity_give_identical_lists(al, sets, expected, monkeypatch, chunk):
    queries, targets = sets
    if chunk is None:
        monkeypatch.delenv("AT_ALLPAIRS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("AT_ALLPAIRS_CHUNK", str(chunk))
    for strands, max_dist, min_sep in (("forward", 12, 0), ("both", 2000, -1)):
        got = al.scan_hits(queries, targets, max_dist, min_sep=min_sep, strands=strands, tile_cols=64)
        assert "resweeps=0;" in al.last_config, al.last_config
        if chunk:
            assert int(al.last_config.split(" slices")[0].split()[-1]) >= len(queries) * len(targets) // chunk
        _same(got, expected(max_dist, min_sep, strands), (chunk, strands))
        one = al.scan_hits(queries, targets, max_dist, min_sep=min_sep, strands=strands, tile_cols=64, cand_cap=1)
        assert int(al.last_config.split("resweeps=")[1].split(";")[0]) >= 1, al.last_config
        for name in ("hit_off", "target", "score", "end_j", "strand"):
            assert np.array_equal(one[name], got[name]), (chunk, strands, name)


@pytest.mark.gpu
@pytest.mark.parametrize("min_sep", [0, 5, -1])
def test_the_best_hit_is_at_scans(al, sets, min_sep):
    queries, targets = sets
    max_dist = 12
    best = al.scan(queries, targets, k=64, strands="both", tile_cols=64)
    got = al.scan_hits(queries, targets, max_dist, min_sep=min_sep, strands="both", tile_cols=64)
    first = {}
    for q in range(len(queries)):
        for e in range(int(got["hit_off"][q]), int(got["hit_off"][q + 1])):
            first.setdefault((q, int(got["strand"][e]), int(got["target"][e])), (int(got["score"][e]), int(got["end_j"][e])))
    n = 0
    for q in range(len(queries)):
        for e in range(int(best["nhits"][q])):
            sc, j = int(best["score"][q, e]), int(best["end_j"][q, e])
            if sc <= min(max_dist, len(queries[q]) - 1) and j >= 1:
                assert first[q, int(best["strand"][q, e]), int(best["target"][q, e])] == (sc, j), (q, e)
                n += 1
    assert n >= 12


def _pack(seqs):
    lens = np.array([len(x) for x in seqs], dtype=np.int32)
    off = np.concatenate(([0], np.cumsum(lens[:-1]))).astype(np.int64) if len(seqs) else np.zeros(0, dtype=np.int64)
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy(), off, lens


@pytest.mark.gpu
def test_two_call_protocol_and_guard_bytes(al, sets):
    queries, targets = sets
    full = al.scan_hits(queries[1:8], targets[5:7], 12, min_sep=0, cigar=True, tile_cols=64)
    nq, nt = 7, 2
    n = int(full["hit_off"][nq])
    total = int(full["cigar_off"][n])
    assert n >= 20 and total > n
    qb, qo, ql = _pack([q.encode() for q in queries[1:8]])
    tb, to, tl = _pack([t.encode() for t in targets[5:7]])
    G, GUARD = 16, 0x5a5a5a5a
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(hit_cap, cigar_cap):
        i32 = {name: np.full(hit_cap + G, GUARD, dtype=np.int32) for name in ("target", "score", "end_j", "strand", "ncigar")}
        off = np.full(nq + 1 + G, GUARD, dtype=np.int64)
        stats = np.full(hit_cap * 8 + G, GUARD, dtype=np.int32)
        coff = np.full(hit_cap + 1 + G, GUARD, dtype=np.int64)
        words = np.full(cigar_cap + G, GUARD, dtype=np.uint32)
        rc = al._lib.at_scan_hits(al._h, nq, p(qb), p(qo), p(ql), nt, p(tb), p(to), p(tl), 12, 0, A.STRAND_FWD, 64, 0, 0, hit_cap, p(off),
                                  p(i32["target"]), p(i32["score"]), p(i32["end_j"]), p(i32["strand"]), p(stats), p(i32["ncigar"]), p(coff),
                                  p(words), cigar_cap)
        assert rc == 0, al._lib.at_last_error(al._h)
        return i32, off, stats, coff, words

    # too few hit entries: the offsets alone, everything else untouched
    i32, off, stats, coff, words = call(n - 1, total)
    assert np.array_equal(off[:nq + 1], full["hit_off"]) and (off[nq + 1:] == GUARD).all()
    assert all((a == GUARD).all() for a in i32.values()) and (stats == GUARD).all() and (coff == GUARD).all() and (words == GUARD).all()
    # room for the hits, and for the words of the first three only
    cap = int(full["cigar_off"][3])
    assert 0 < cap < total
    i32, off, stats, coff, words = call(n, cap)
    assert np.array_equal(off[:nq + 1], full["hit_off"]) and (off[nq + 1:] == GUARD).all()
    for name in ("target", "score", "end_j", "strand", "ncigar"):
        assert np.array_equal(i32[name][:n], full[name]) and (i32[name][n:] == GUARD).all(), name
    assert np.array_equal(stats[:n * 8], full["stats"].reshape(-1)) and (stats[n * 8:] == GUARD).all()
    assert np.array_equal(coff[:n + 1], full["cigar_off"]) and (coff[n + 1:] == GUARD).all()          # counts and offsets are complete
    flat = np.concatenate(full["cigar"])
    assert np.array_equal(words[:cap], flat[:cap]) and (words[cap:] == GUARD).all()


@pytest.mark.gpu
def test_refusals_and_empty_sets(al, sets, expected):
    queries, targets = sets
    q, t = queries[:4], targets[4:6]
    two = A.Aligner()
    try:
        two.set_scoring(1, 2, -5, -1, -10)
        with pytest.raises(A.AlignToolsError) as ei:
            two.scan_hits(q, t, 3)
        assert ei.value.code == A.ERR_DOMAIN and "u = 2, not 1" in str(ei.value), ei.value
    finally:
        two.close()
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_hits(q, t + ["ACGTNACGT" * 30], 3)
    assert ei.value.code == A.ERR_DOMAIN and "ACGT" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_hits(q + ["ACGTA" * 205], t, 3)
    assert ei.value.code == A.ERR_DOMAIN and "1025 bases, more than 1024" in str(ei.value), ei.value
    for kw, text in ((dict(max_dist=-1), "max_dist = -1"), (dict(max_dist=3, min_sep=-2), "min_sep = -2"),
                     (dict(max_dist=3, cand_cap=-1), "negative capacity"), (dict(max_dist=3, tile_cols=24), "tile_cols = 24")):
        with pytest.raises(A.AlignToolsError) as ei:
            al.scan_hits(q, t, **kw)
        assert ei.value.code == A.ERR_ARG and text in str(ei.value), ei.value
    with pytest.raises(ValueError):
        al.scan_hits(q, t, 3, strands="sideways")
    off = np.zeros(5, dtype=np.int64)
    rc = al._lib.at_scan_hits(al._h, 0, None, None, None, 0, None, None, None, 3, 0, 7, 0, 0, 0, 0, off.ctypes.data_as(C.c_void_p),
                              None, None, None, None, None, None, None, None, 0)
    assert rc == A.ERR_ARG and b"strands = 7" in al._lib.at_last_error(al._h)
    rc = al._lib.at_scan_hits(al._h, 0, None, None, None, 0, None, None, None, 3, 0, A.STRAND_FWD, 0, 0, 0, -1, off.ctypes.data_as(C.c_void_p),
                              None, None, None, None, None, None, None, None, 0)
    assert rc == A.ERR_ARG
    # no queries, no targets: complete offsets, no hits
    got = al.scan_hits([], targets, 3, cigar=True)
    assert list(got["hit_off"]) == [0] and len(got["target"]) == 0 and len(got["cigar"]) == 0
    got = al.scan_hits(q, [], 3, cigar=True)
    assert list(got["hit_off"]) == [0] * 5 and len(got["target"]) == 0 and al.last_config.startswith("scan-hits: ")
    # a query of length 0 has no hits; the handle works afterwards and its settings are what they were
    got = al.scan_hits([""] + queries, targets, 12, min_sep=0, tile_cols=64)
    _same(got, [[]] + expected(12, 0, "forward"), "after the refusals")
    on = A.Aligner()
    try:
        on.set_scoring(*UNIT)
        on.set_edit_infix(True)
        on.set_edit_traceback(True)
        a = al.scan_hits(queries[:8], targets, 12, strands="both", cigar=True)
        b = on.scan_hits(queries[:8], targets, 12, strands="both", cigar=True)
        for name in ("hit_off", "target", "score", "end_j", "strand", "ncigar", "stats", "cigar_off"):
            assert np.array_equal(a[name], b[name]), name
        pair = [(queries[3], targets[5])]
        r = al.align_batch("edit", pair)
        assert "infix" not in al.last_config and "ops" not in r and int(r["end_j"][0]) == len(targets[5])
        r = on.align_batch("edit", pair)
        row = _table(queries[3].encode(), targets[5].encode(), True)[2][len(queries[3])]
        assert "infix" in on.last_config and "ops" in r and (int(r["score"][0]), int(r["end_j"][0])) == (int(row.min()), int(np.argmin(row)))
    finally:
        on.close()
