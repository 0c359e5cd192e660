"""at_scan_local / Aligner.scan_local: Smith-Waterman of reads against long targets.

Nothing new is defined: a hit is what align_batch("local") returns for (query or its reverse complement, whole target), so every
expected value is oracle.align(LOCAL, ...) on the whole target, ranked by the rule of at_search_strands.

On the CPU: the exports, the Python-side argument errors and the two facts that make the tiling exact -- the tile fact (with and
without a cutoff) and the window fact -- as a pure Python driver over oracle.align with the planner's own numbers, plus a control
with an overlap of 16 columns that must go wrong.  On the GPU every hit is compared in full."""
import random

import numpy as np
import pytest

import aligntools.c_amd as A
import oracle as O

LOCAL = O.MODE_NAMES["local"]
SCORINGS = [(2, -2, -5, -2), (1, -2, -5, -1), (5, -4, -10, -1), (3, -1, -1, -3)]
CPU_SCORINGS = SCORINGS + [(1, -1, -2, -2), (4, 1, -3, -1)]
NAMES = ("target", "score", "end_i", "end_j", "state", "nhits")
STRANDS_OF = {"forward": (0,), "reverse": (1,), "both": (0, 1)}


def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _rc(s):
    return A.revcomp(s).decode("latin1")


def _sw(q, t, sc):
    r = O.align(LOCAL, q, t, sc[0], sc[1], sc[2], sc[3])
    assert r["rc"] == 0
    return r


@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


# ---------------------------------------------------------------- CPU: exports, the planner's export, argument errors

def test_symbols_exported(lib):
    for name in ("at_scan_local", "at_scan_local_plan", "at_scan_local_window"):
        assert name in A.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    assert callable(A.Aligner.scan_local) and callable(A.scan_local_plan)


def test_plan_export(lib):
    # 150 rows, 2/-2/-5/-2: g = floor((300 - 1) / 2) = 149, ov = round16up(299) = 304
    assert A.scan_local_plan(150, 300000, 2, -2, -5, -2) == (1024, 304, 293, 292)
    assert A.scan_local_plan(150, 300000, 2, -2, -5, -2, min_score=200) == (1024, 208, 293, 292)
    assert A.scan_local_plan(150, 300000, 2, -2, -5, -2, tile_cols=2048) == (2048, 304, 147, 146)
    assert A.scan_local_plan(150, 2048 * 3, 2, -2, -5, -2, tile_cols=2048)[2:] == (3, 3)
    assert A.scan_local_plan(20, 100, 2, -2, -5, -2, tile_cols=16) == (16, 48, 7, 6)
    assert A.scan_local_plan(20, 60, 2, -2, -5, -2, tile_cols=16)[2:] == (4, 0)           # a target shorter than one full tile
    for bad in (24, 8, -16, 1000):
        with pytest.raises(A.AlignToolsError) as ei:
            A.scan_local_plan(100, 1000, 2, -2, -5, -2, tile_cols=bad)
        assert ei.value.code == A.ERR_ARG and "multiple of 16" in str(ei.value)
    for m, u, o, e, l1 in ((0, -2, -5, -2, 10), (2, -2, 0, -2, 10), (2, -2, -5, 0, 10), (2, -2, -5, -2, 1025), (2, -2, -5, -2, 0), (1024, 0, -1, -1, 1024)):
        with pytest.raises(A.AlignToolsError) as ei:
            A.scan_local_plan(l1, 1000, m, u, o, e)
        assert ei.value.code == A.ERR_DOMAIN, (m, u, o, e, l1)


def test_python_side_argument_errors():
    al = object.__new__(A.Aligner)                              # no handle: both errors come before the library is asked
    al._h = None
    with pytest.raises(ValueError):
        al.scan_local(["ACGT"], ["ACGT"], strands="sideways")
    with pytest.raises(TypeError):
        al.scan_local(["ACGT"], ["ACGT"], cutoff=3)             # the bound is called min_score here
    import inspect
    assert str(inspect.signature(A.Aligner.scan_local)) == \
        "(self, queries, targets, k=1, min_score=None, strands='forward', cigar=False, cigar_m=False, tile_cols=0)"
    # the existing method is as it was
    assert str(inspect.signature(A.Aligner.scan)) == "(self, queries, targets, k=1, cutoff=None, strands='forward', cigar=False, cigar_m=False, tile_cols=0)"


# ---------------------------------------------------------------- CPU: the facts, on the oracle

def _tiles(l1, l2, sc, min_score, tile_cols, ov_override=None):
    """[(s0, e)] of every tile: it sweeps the target columns (s0, e]"""
    T, ov, ntiles, nfull = A.scan_local_plan(l1, l2, sc[0], sc[1], sc[2], sc[3], min_score, tile_cols)
    out = []
    dropped = min(ntiles - 1, ov // T) if ov_override is None else 0      # the tiles 1 .. dropped would repeat tile 0's sweep: not swept
    for n in range(ntiles):
        if 1 <= n <= dropped:
            assert max(0, n * T - ov) == 0 and min(l2, (n + 1) * T) <= min(l2, T + ov)
            continue
        if ov_override is None:
            s0 = max(0, n * T - ov)
            e = min(l2, s0 + T + ov)
            assert (e - s0 == T + ov) == (n < nfull) and e >= min(l2, (n + 1) * T) and s0 % 16 == 0
        else:                                                  # the control: too little in front, nothing behind
            s0, e = max(0, n * T - ov_override), min(l2, (n + 1) * T)
        out.append((s0, e))
    return out


def _tile_merge(q, t, sc, min_score, tile_cols, ov_override=None):
    """the lexicographic minimum of (-score, end_i, s0 + end_j) over the tiles, each swept as an ordinary local pair"""
    best = None
    for s0, e in _tiles(len(q), len(t), sc, min_score, tile_cols, ov_override):
        r = _sw(q, t[s0:e], sc)
        key = (-r["score"], r["end_i"], s0 + r["end_j"])
        best = key if best is None or key < best else best
    return (-best[0], best[1], best[2])


def _fact_pairs(n_pairs, seed):
    rng = random.Random(seed)
    pairs = []
    for n in range(n_pairs):
        alpha = ("ACGT", "ACGT", "AC", "A")[n % 4]
        l1 = rng.randint(1, 64)
        l2 = rng.choice((1, 15, 16, 17, 33)) if n % 17 == 0 else rng.randint(1, 1500)
        q = _rnd(rng, l1, alpha)
        t = list(_rnd(rng, l2, alpha if n % 5 else "ACGT"))
        for _ in range(rng.randint(0, 3) if n % 3 else 0):     # planted copies carrying substitutions and indels
            body = list(q)
            for _ in range(rng.randint(0, 3)):
                body[rng.randrange(len(body))] = rng.choice("ACGT")
            for _ in range(rng.randint(0, 2)):
                x = rng.randrange(len(body))
                if rng.random() < 0.5 and len(body) > 4:
                    del body[x:x + rng.randint(1, 3)]
                else:
                    body[x:x] = list(_rnd(rng, rng.randint(1, 4)))
            at = rng.randint(0, max(0, l2 - len(body)))
            t[at:at + len(body)] = body
        t = "".join(t)[:max(l2, 1)]
        pairs.append((q, t, CPU_SCORINGS[n % 6], (16, 32, 64, 256)[(n // 6) % 4]))
    return pairs


def test_tile_fact():
    pairs = _fact_pairs(420, 2016)
    pairs += [("A" * l1, "CGT" * l2, sc, T) for l1, l2, sc, T in ((1, 1, SCORINGS[0], 16), (7, 200, SCORINGS[1], 16), (64, 400, SCORINGS[2], 32),
                                                               (30, 333, SCORINGS[3], 64), (5, 90, CPU_SCORINGS[4], 256))]
    zero = 0
    for q, t, sc, T in pairs:
        r = _sw(q, t, sc)
        assert _tile_merge(q, t, sc, None, T) == (r["score"], r["end_i"], r["end_j"]), (q, t, sc, T)
        zero += r["score"] == 0
        if r["score"] == 0:
            assert (r["end_i"], r["end_j"]) == (1, 1)           # no positive cell: the first cell, in every tiling
    assert zero >= 5


def test_tile_fact_with_a_cutoff():
    pairs = _fact_pairs(480, 2017)
    under = 0
    for n, (q, t, sc, T) in enumerate(pairs):
        r = _sw(q, t, sc)
        cutoff = (max(sc[0], sc[1]) * len(q) * (1 + n % 4)) // 4
        got = _tile_merge(q, t, sc, cutoff, T)
        if r["score"] >= max(1, cutoff):
            assert got == (r["score"], r["end_i"], r["end_j"]), (q, t, sc, T, cutoff)
        else:
            under += 1
            assert got[0] < max(1, cutoff) and got[0] <= r["score"], (q, t, sc, T, cutoff, got)   # no false hit
    assert under >= 40


def test_window_fact():
    pairs = _fact_pairs(240, 2018)
    cut = 0
    for q, t, sc, _T in pairs:
        r = _sw(q, t, sc)
        ws = A.scan_local_window(r["end_i"], r["end_j"], r["score"], *sc)
        assert ws % 16 == 0 and 0 <= ws <= r["end_j"]
        cut += ws > 0
        w = _sw(q, t[ws:r["end_j"]], sc)
        assert (w["score"], w["end_i"], w["end_j"], w["state"]) == (r["score"], r["end_i"], r["end_j"] - ws, r["state"]), (q, t, sc)
        assert w["ops"] == r["ops"], (q, t, sc)
    assert cut >= 60                                            # the windows do cut targets


def test_control_overlap_of_16_goes_wrong():
    pairs = _fact_pairs(240, 2016)
    wrong = 0
    for q, t, sc, T in pairs:
        r = _sw(q, t, sc)
        wrong += _tile_merge(q, t, sc, None, T, ov_override=16) != (r["score"], r["end_i"], r["end_j"])
    assert wrong >= 10, wrong                                   # the inputs do discriminate


# ---------------------------------------------------------------- GPU

QLENS = (1, 19, 20, 38, 39, 76, 77, 150, 151, 256, 257, 608, 609, 1024)      # the row-class edges of the packed kernels


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


@pytest.fixture(scope="module")
def sets():
    """queries at the class edges; targets of a few thousand bases with copies planted as given, reverse-complemented, with
    substitutions and indels: ending on an own-range start of every width (a multiple of 2 048), one column before and one after it,
    starting in column 1, ending in column l2, and the same exact copy in several tiles"""
    rng = random.Random(1616)
    queries = [_rnd(rng, n) for n in QLENS]

    def plant(t, q, end):
        assert end - len(q) >= 0 and end <= len(t)
        t[end - len(q):end] = q

    a, b, c = list(_rnd(rng, 4500)), list(_rnd(rng, 2101)), list(_rnd(rng, 6200))
    plant(a, queries[7], 150)                                   # starts in column 1
    plant(a, queries[5], 2048); plant(a, queries[6], 2047 - 76); plant(a, _rc(queries[8]), 2049 + 151 + 100)
    plant(a, _mutate(rng, queries[9], 6, 1, 1), 3100); plant(a, queries[10], 4500)      # ends in column l2
    plant(b, queries[3], 64); plant(b, queries[4], 65 + 39); plant(b, queries[2], 63 + 39 + 40 + 20)
    plant(b, _rc(_mutate(rng, queries[11], 12, 2, 1)), 1500); plant(b, _mutate(rng, queries[8], 3, 1, 0), 2101)
    for end in (700, 2048 + 608 + 11, 4096 + 609, 6200):        # the same exact copy in several tiles: the tie goes to the first
        plant(c, queries[11], end)
    plant(c, _mutate(rng, queries[13], 30, 3, 2), 1900)
    plant(c, _rc(queries[12]), 3400 + 609)
    n_run = "N" * 300 + queries[7] + "N" * 500 + _mutate(rng, queries[9], 4, 0, 1) + "N" * 200
    targets = ["".join(a), "".join(b), "".join(c), n_run, _rnd(rng, 30), "".join(a), "A" * 2300]
    queries.append("A" * 70)                                    # poly-A in poly-A
    queries.append("ACGT" * 10 + "N" * 5 + "ACGT" * 5)          # a read with N
    return queries, targets


def _brute(queries, targets, sc, strands=(0, 1)):
    nq, nt = len(queries), len(targets)
    seqs = [queries, [_rc(q) for q in queries]]
    full = {name: np.zeros((nq, 2, nt), dtype=np.int64) for name in ("score", "end_i", "end_j", "state")}
    ops = {}
    for q in range(nq):
        for s in strands:
            for t in range(nt):
                r = _sw(seqs[s][q], targets[t], sc)
                for name in full:
                    full[name][q, s, t] = r[name]
                ops[q, s, t] = r["ops"]
    return full, ops


_BRUTE = {}


def _brute_of(sets, sc, strands=(0, 1)):
    key = (sc, strands)
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
        cand = [(t, s) for t in range(nt) for s in strands]
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
@pytest.mark.parametrize("sc", SCORINGS, ids=["2-2-5-2", "1-2-5-1", "5-4-10-1", "3-1-1-3"])
def test_lists_equal_the_oracle_on_the_whole_target(al, sets, sc, tile_cols):
    queries, targets = sets
    first = sc == SCORINGS[0]
    strands = "both" if first else "forward"
    full_ops = _brute_of(sets, sc, (0, 1) if first else (0,))
    al.set_scoring(sc[0], sc[1], sc[2], sc[3])
    for k in ((1, 3, 64) if first or tile_cols == 64 else (3,)):
        cg = k == 3
        got = al.scan_local(queries, targets, k=k, strands=strands, tile_cols=tile_cols, cigar=cg, cigar_m=cg and tile_cols == 64)
        cfg = al.last_config
        assert cfg.startswith("local-scan: tile=%d " % (tile_cols or 1024)) and " tiles=" in cfg and " slices; " in cfg, cfg
        if tile_cols == 16:
            assert int(cfg.split("tiles=")[1].split()[0]) > 100 * len(targets)      # many tiles per target
        _same(got, _expected(full_ops[0], STRANDS_OF[strands], k, None), NAMES + (("strand",) if strands == "both" else ()), (sc, tile_cols, k))
        if cg:
            assert "; windows: " in cfg, cfg
            _check_cigars(got, queries, targets, full_ops, tile_cols == 64)


@pytest.mark.gpu
def test_placements_and_ties(al, sets):
    queries, targets = sets
    sc = SCORINGS[0]
    full, _ops = _brute_of(sets, sc)
    # the planted copies are where the fixture put them (exact copies score 2 * length)
    for q, t, end in ((7, 0, 150), (5, 0, 2048), (10, 0, 4500), (3, 1, 64), (11, 2, 700), (7, 3, 450)):
        assert (full["score"][q, 0, t], full["end_i"][q, 0, t], full["end_j"][q, 0, t]) == (2 * QLENS[q], QLENS[q], end), (q, t)
    assert full["score"][8, 1, 0] == 2 * 151 and full["end_j"][8, 1, 0] == 2049 + 151 + 100
    assert (full["score"][14, 0, 6], full["end_i"][14, 0, 6], full["end_j"][14, 0, 6]) == (140, 70, 70)   # poly-A: the first cell that has it
    assert len(queries[13]) > len(targets[4])                   # a read longer than its target
    al.set_scoring(*sc)
    for tile_cols in (16, 64, 0):
        got = al.scan_local(queries, targets, k=7, strands="both", tile_cols=tile_cols)
        _same(got, _expected(full, (0, 1), 7, None), NAMES + ("strand",), tile_cols)
        assert list(got["target"][7, :3]) == [0, 3, 5] and list(got["end_j"][7, :3]) == [150, 450, 150]   # equal scores: the smaller index first


@pytest.mark.gpu
def test_all_mismatch_pair(al):
    al.set_scoring(2, -2, -5, -2)
    for tile_cols in (16, 0):
        got = al.scan_local(["A" * 40, "C" * 7], ["G" * 700, "T" * 5], k=2, tile_cols=tile_cols, cigar=True)
        assert (got["score"] == 0).all() and (got["end_i"] == 1).all() and (got["end_j"] == 1).all() and (got["state"] == A.ST_MID).all()
        assert (got["target"] == [[0, 1], [0, 1]]).all() and (got["nhits"] == 2).all()
        r = _sw("A" * 40, "G" * 700, (2, -2, -5, -2))
        assert (r["score"], r["end_i"], r["end_j"]) == (0, 1, 1)
        words, stats = A.cigar(r["ops"], "A" * 40, 1, "G" * 700, 1)
        assert np.array_equal(got["cigar"][0][0], words) and np.array_equal(got["stats"][0, 0], stats)


@pytest.mark.gpu
@pytest.mark.parametrize("strands", ["forward", "reverse", "both"])
def test_equals_search_local(al, sets, strands):
    queries, targets = sets
    al.set_scoring(*SCORINGS[0])
    for k, min_score in ((1, None), (5, None), (64, 60)):
        want = al.search("local", queries, targets, k=k, cutoff=min_score, strands=strands)
        for tile_cols in (64, 0):
            got = al.scan_local(queries, targets, k=k, min_score=min_score, strands=strands, tile_cols=tile_cols)
            _same(got, want, NAMES + (("strand",) if strands != "forward" else ()), (strands, k, min_score, tile_cols))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, None])
def test_slices_give_identical_lists(al, monkeypatch, chunk):
    """AT_ALLPAIRS_CHUNK = 1: one tile pair per slice, a pair's slot lives through all of them"""
    rng = random.Random(3)
    queries = [_rnd(rng, n) for n in (20, 39, 77, 20, 257)]
    body = list(_rnd(rng, 700))
    body[100:120] = queries[0]; body[340:379] = queries[1]; body[600:677] = _rc(queries[2])
    wide = list(_rnd(rng, 2600))
    wide[900:1157] = queries[4]                                # across the first own-range end of the default width
    targets = ["".join(body), _rnd(rng, 90), queries[3] + _rnd(rng, 200), "".join(wide)]
    sc = SCORINGS[0]
    full_ops = _brute(queries, targets, sc)
    if chunk is None:
        monkeypatch.delenv("AT_ALLPAIRS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("AT_ALLPAIRS_CHUNK", str(chunk))
    al.set_scoring(*sc)
    got = al.scan_local(queries, targets, k=3, strands="both", tile_cols=64, cigar=True)
    if chunk is not None:
        cfg = al.last_config
        tiles, slices = int(cfg.split("tiles=")[1].split()[0]), int(cfg.split(" blocks, ")[1].split()[0])
        assert tiles > 100 and (slices == tiles if chunk == 1 else slices >= -(-tiles // 7)), cfg
    _same(got, _expected(full_ops[0], (0, 1), 3, None), NAMES + ("strand",), chunk)
    _check_cigars(got, queries, targets, full_ops, False)
    # the default width: full-shape tiles of 257 x (1 024 + ov) and the shorter ones behind them, one pair per slice
    got = al.scan_local(queries, targets, k=3, strands="both", cigar=True)
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
        got = al.scan_local(queries[:8], targets[:3], k=4, min_score=40, strands="both", cigar=True, tile_cols=256)
        if piece is not None:
            assert " %d pieces, " % -(-int(got["nhits"].sum()) // piece) in al.last_config, al.last_config
        n = got["target"].size
        assert 0 < int(got["nhits"].sum()) < n                  # used and unused entries
        off, nc = got["cigar_off"], got["ncigar"].reshape(-1)
        assert off[0] == 0 and np.array_equal(off[1:] - off[:-1], nc) and (nc[got["target"].reshape(-1) < 0] == 0).all()
        sub = {name: full_ops[0][name][:8, :, :3] for name in full_ops[0]}
        _same(got, _expected(sub, (0, 1), 4, 40), NAMES + ("strand",), piece)
        _check_cigars(got, queries[:8], targets, full_ops, False)
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
    for min_score in (30, 120, 400):
        want = _expected(full, (0, 1), 4, min_score)
        assert 0 < want["nhits"].sum() < 4 * len(queries)
        for tile_cols in (64, 0):
            got = al.scan_local(queries, targets, k=4, min_score=min_score, strands="both", tile_cols=tile_cols)
            _same(got, want, NAMES + ("strand",), (min_score, tile_cols))


@pytest.mark.gpu
def test_min_score_setting_neither_matters_nor_changes(al, sets):
    queries, targets = sets
    al.set_scoring(*SCORINGS[0])
    a = al.scan_local(queries[:6], targets[:3], k=2, tile_cols=64)
    al.set_min_score(500)
    try:
        b = al.scan_local(queries[:6], targets[:3], k=2, tile_cols=64)
    finally:
        al.set_min_score(None)
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
def test_edges_and_refusals(al, sets):
    queries, targets = sets
    q, t = queries[:4], targets[:2]
    al.set_scoring(*SCORINGS[0])
    got = al.scan_local([], t, k=2)
    assert got["target"].shape == (0, 2)
    got = al.scan_local(q, [], k=2, cigar=True)
    assert (got["nhits"] == 0).all() and (got["target"] == -1).all() and (got["ncigar"] == 0).all() and (got["stats"] == -1).all()
    for k in (0, 65):
        with pytest.raises(A.AlignToolsError) as ei:
            al.scan_local(q, t, k=k)
        assert ei.value.code == A.ERR_ARG and "k = %d outside 1..64" % k in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_local(q, t, tile_cols=24)
    assert ei.value.code == A.ERR_ARG and "multiple of 16" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan_local(q + ["ACGTA" * 205], t)
    assert ei.value.code == A.ERR_DOMAIN and "1025 bases" in str(ei.value), ei.value
    for bad_q, bad_t in ((q + [""], t), (q, t + [""])):
        with pytest.raises(A.AlignToolsError) as ei:
            al.scan_local(bad_q, bad_t)
        assert ei.value.code == A.ERR_DOMAIN and "empty" in str(ei.value), ei.value
    for m, u, o, e in ((2, -2, -5, 0), (0, -2, -5, -2), (2, -2, 0, -2)):
        other = A.Aligner(0)
        try:
            other.set_scoring(m, u, o, e)
            with pytest.raises(A.AlignToolsError) as ei:
                other.scan_local(q, t)
            assert ei.value.code == A.ERR_DOMAIN and "m >= 1, o <= -1 and e <= -1" in str(ei.value), ei.value
        finally:
            other.close()
    # a tile is a pair of the batch entry: its exact-score bound is said up front (200 * (1 024 + 1 024 + ov + 2) >= 2^24, ov > 200 000)
    other = A.Aligner(0)
    try:
        other.set_scoring(200, -1, -1, -1)
        with pytest.raises(A.AlignToolsError) as ei:
            other.scan_local([queries[13]], t)
        assert ei.value.code == -3 and "exact score range" in str(ei.value), ei.value
        got = other.scan_local([queries[1]], [targets[1]])      # 19 bases: inside the bound
        r = _sw(queries[1], targets[1], (200, -1, -1, -1))
        assert (int(got["score"][0, 0]), int(got["end_i"][0, 0]), int(got["end_j"][0, 0])) == (r["score"], r["end_i"], r["end_j"])
    finally:
        other.close()
    # the handle works afterwards
    full, _ops = _brute_of(sets, SCORINGS[0])
    got = al.scan_local(queries, targets, k=2, tile_cols=64)
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
            other.scan_local(["ACGT"], ["ACGTACGT"])
        assert ei.value.code == A.ERR_DOMAIN and "one GPU only" in str(ei.value), ei.value
    finally:
        other.close()


@pytest.mark.gpu
def test_eight_reads_in_300k(al):
    rng = random.Random(300000)
    body = list(_rnd(rng, 300000))
    reads, ends = [], []
    for x, end in enumerate((150, 2048, 40961, 100000, 150000 + 77, 204800 + 149, 262145, 300000)):
        r = _rnd(rng, 150)
        body[end - 150:end] = r
        reads.append(r if x % 2 == 0 else _rc(r))
        ends.append(end)
    target = "".join(body)
    al.set_scoring(*SCORINGS[0])
    got = al.scan_local(reads, [target], k=1, strands="both", cigar=True)
    assert "local-scan: tile=1024 overlap<=304 tiles=%d " % (293 * 16) in al.last_config, al.last_config
    assert (got["nhits"] == 1).all() and (got["score"][:, 0] == 300).all() and (got["end_i"][:, 0] == 150).all()
    assert list(got["end_j"][:, 0]) == ends and list(got["strand"][:, 0]) == [0, 1] * 4
    assert [A.cigar_string(w[0]) for w in got["cigar"]] == [b"150="] * 8
    assert list(got["stats"][:, 0, 1]) == [e - 150 for e in ends]          # AT_CG_START_J is absolute
