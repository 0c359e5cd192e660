"""at_scan / Aligner.scan: reads against long targets -- the rule of edit infix mode with no bound on the target length.

Nothing new is defined: a hit is what at_search_strands delivers under at_set_edit_infix, so every expected value comes from the
restatement of tests/test_edit_infix.py (_infix_ref on the FULL table of (query or its reverse complement, target)) and the
brute-force ranking of tests/test_search_infix.py (_expected).

On the CPU: the exports, the planner (at_scan_plan) and the two facts that make the tiling exact, checked on the
numpy restatement with the planner's own numbers.  On the GPU every hit is compared in full."""
import ctypes as C
import random

import numpy as np
import pytest

import aligntools.c_amd as A
from test_edit_infix import _global_ref, _infix_ref, _table
from test_search_infix import NAMES, STRANDS_OF, _expected, _same
from test_search_infix import sets as infix_sets          # noqa: F401  (the query and target sets of the infix search tests)

UNIT = (1, 1, -5, -1, -10)
CUTOFFS = (None, 0, 3, 12)
WIDTHS = (16, 48, 256)


def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _rc(s):
    return A.revcomp(s).decode("latin1")


# ---------------------------------------------------------------- CPU: exports and the planner

@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


def test_scan_symbols_exported(lib):
    for name in ("at_scan", "at_scan_plan"):
        assert name in A.ABI_SYMBOLS
        assert getattr(lib, name) is not None


def _c_of(l1, cutoff):
    return l1 if cutoff is None else max(0, min(l1, cutoff))


def _tiles(l1, l2, cutoff, tile_cols):
    """[(s0, own0, e)] of every lane-tile that has columns: it sweeps (s0, e] and owns (own0, e]"""
    T, ov, ng = A.scan_plan(l1, l2, cutoff, tile_cols)
    out = []
    for n in range(64 * ng):
        s0, e = max(0, n * T - ov), min((n + 1) * T, l2)
        if e > n * T:
            out.append((s0, n * T, e))
    return T, ov, ng, out


def test_planner_properties(lib):
    rng = random.Random(5)
    cases = []
    for T in (16, 48, 256, 1024):
        for l2 in (0, 1, 64 * T - 1, 64 * T, 64 * T + 1):
            for l1 in (1, 1024):
                cases.append((l1, l2, rng.choice(CUTOFFS), T))
    for _ in range(300):
        cases.append((rng.randint(0, 1024), rng.randint(0, 400000), rng.choice(CUTOFFS + (5000, -2)), rng.choice((0, 16, 32, 48, 256, 4096))))
    for l1, l2, cutoff, tile_cols in cases:
        T, ov, ng, tiles = _tiles(l1, l2, cutoff, tile_cols)
        assert T == (tile_cols or T) and T % 16 == 0 and T > 0
        assert ov % 16 == 0 and l1 + _c_of(l1, cutoff) <= ov < l1 + _c_of(l1, cutoff) + 16
        assert ng == max(1, -(-l2 // (64 * T)))
        # the own ranges cover the columns 1 .. l2 exactly once, in order, and every sweep starts on a packed word
        at = 0
        for s0, own0, e in tiles:
            assert own0 == at and e > own0 and s0 % 16 == 0 and s0 == max(0, own0 - ov)
            at = e
        assert at == l2
    # the default is one documented value
    assert len({A.scan_plan(l1, l2)[0] for l1 in (1, 150, 1024) for l2 in (0, 10, 10 ** 6)}) == 1


@pytest.mark.parametrize("tile_cols", [24, 8, -16, 1000])
def test_planner_refuses_bad_widths(lib, tile_cols):
    with pytest.raises(A.AlignToolsError) as ei:
        A.scan_plan(100, 1000, None, tile_cols)
    assert ei.value.code == A.ERR_ARG and "multiple of 16" in str(ei.value)


# ---------------------------------------------------------------- CPU: the two facts, on the restatement

def _fact_pairs():
    rng = random.Random(1912)
    pairs = []
    for n in range(312):
        alpha = ("ACGT", "ACGT", "AC", "A")[n % 4]
        l1 = rng.randint(1, 60) if n % 13 else rng.randint(100, 150)
        l2 = rng.choice((0, 1, 15, 16, 17)) if n % 17 == 0 else rng.randint(0, 700)
        q = _rnd(rng, l1, alpha)
        t = list(_rnd(rng, l2, alpha))
        if n % 3 and l2:                                       # planted, with a few edits
            body = list(q)
            for _ in range(rng.randint(0, 4)):
                body[rng.randrange(len(body))] = rng.choice(alpha)
            if rng.random() < 0.4 and len(body) > 1:
                del body[rng.randrange(len(body))]
            at = rng.randint(0, max(0, l2 - len(body)))
            t[at:at + len(body)] = body
            t = t[:l2]
        pairs.append((q.encode(), "".join(t).encode(), WIDTHS[n % 3], CUTOFFS[(n // 3) % 4]))
    return pairs


def _tile_merge(q, t, cutoff, tile_cols):
    """the lexicographic minimum of (score, absolute column) over the candidate (l1, 0) and every column of every tile's own sweep --
    warm-up columns included, as the kernel does"""
    l1, l2 = len(q), len(t)
    _T, _ov, _ng, tiles = _tiles(l1, l2, cutoff, tile_cols)
    best = (l1, 0)
    for s0, _own0, e in tiles:
        _a, _b, D = _table(q, t[s0:e], True)
        row = D[l1]
        j = int(np.argmin(row[1:])) + 1
        best = min(best, (int(row[j]), s0 + j), (l1, s0))
    return best


def test_tiles_and_window_are_exact():
    pairs = _fact_pairs()
    assert len(pairs) >= 300
    above = 0
    for q, t, T, cutoff in pairs:
        d, js, ops, j0 = _infix_ref(q, t)
        c = _c_of(len(q), cutoff)
        got = _tile_merge(q, t, cutoff, T)
        if d <= c:
            assert got == (d, js), (len(q), len(t), T, cutoff, got, (d, js))
        else:
            above += 1
            assert got[0] > c, (len(q), len(t), T, cutoff, got, d)
        # the window: (read, target columns (ws, j*]) has the same score, its end column is j* - ws, its ops are byte for byte the same
        ws = max(0, (js - len(q) - d) & ~15) if js - len(q) - d > 0 else 0
        assert _infix_ref(q, t[ws:js]) == (d, js - ws, ops, j0 - ws), (len(q), len(t), ws, js)
    assert above >= 20


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    a.set_scoring(*UNIT)
    yield a
    a.close()


QLENS = (1, 31, 32, 33, 64, 65, 128, 129, 160, 161, 256, 257, 512, 513, 1024)


@pytest.fixture(scope="module")
def long_sets():
    """queries at the class edges; targets of 0, 1, 15..17, ~1 000, ~2 100 and ~9 000 bases with exact copies planted so that j* falls
    on an own-range start of every width, one before and one after it, on a group boundary (T = 16: 1 024, T = 64: 4 096) and with a
    copy spanning one"""
    rng = random.Random(77)
    queries = [_rnd(rng, n) for n in QLENS]
    queries[4] = _rc(queries[4][:32]) + queries[4][:32]      # equal to its own reverse complement
    assert _rc(queries[4]) == queries[4]

    def plant(t, q, end):
        assert end - len(q) >= 0 and end <= len(t)
        t[end - len(q):end] = q

    t1k, t2k, t9k = list(_rnd(rng, 1003)), list(_rnd(rng, 2101)), list(_rnd(rng, 9001))
    plant(t1k, queries[2], 512); plant(t1k, queries[3], 769); plant(t1k, _rc(queries[5]), 1003)
    plant(t2k, queries[6], 1024); plant(t2k, queries[7], 1279); plant(t2k, queries[5], 1535); plant(t2k, queries[8], 2049)
    plant(t9k, queries[1], 1040); plant(t9k, queries[13], 2304); plant(t9k, queries[10], 2560); plant(t9k, queries[9], 3000)
    plant(t9k, queries[11], 4300); plant(t9k, _rc(queries[12]), 8200)
    mut = list(queries[14])
    for x in (3, 500, 1000):
        mut[x] = "ACGT"[("ACGT".index(mut[x]) + 1) % 4]
    del mut[700]
    plant(t9k, mut, 6000)
    targets = ["", _rnd(rng, 1), _rnd(rng, 15), _rnd(rng, 16), _rnd(rng, 17), "".join(t1k), "".join(t2k), "".join(t9k)]
    return queries, targets


def _brute(queries, targets):
    nq, nt = len(queries), len(targets)
    seqs = [queries, [_rc(q) for q in queries]]
    full = {name: np.zeros((nq, 2, nt), dtype=np.int64) for name in ("score", "end_i", "end_j", "state")}
    for a in range(nq):
        for s in (0, 1):
            for b in range(nt):
                d, js, _ops, _j0 = _infix_ref(seqs[s][a].encode(), targets[b].encode())
                full["score"][a, s, b], full["end_i"][a, s, b], full["end_j"][a, s, b], full["state"][a, s, b] = d, len(queries[a]), js, A.ST_MID
    return full


@pytest.fixture(scope="module")
def long_brute(long_sets):
    return _brute(*long_sets)


def _check_cigars(got, queries, targets, merge):
    nq, k = got["target"].shape
    for q in range(nq):
        for e in range(k):
            t = int(got["target"][q, e])
            if t < 0:
                assert int(got["ncigar"][q, e]) == 0 and (got["stats"][q, e] == -1).all() and len(got["cigar"][q][e]) == 0
                continue
            s1 = queries[q] if int(got.get("strand", np.zeros((nq, k)))[q, e]) == 0 else _rc(queries[q])
            d, js, ops, _j0 = _infix_ref(s1.encode(), targets[t].encode())
            words, stats = A.cigar(ops, s1, len(s1), targets[t], js, extended=not merge)
            assert int(got["ncigar"][q, e]) == len(words), (q, e)
            assert np.array_equal(got["cigar"][q][e], words), (q, e)
            assert np.array_equal(got["stats"][q, e], stats), (q, e, got["stats"][q, e], stats)


@pytest.mark.gpu
@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("cutoff", [None, 12], ids=["all", "cutoff12"])
@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("tile_cols", [16, 64, 256, 0])
def test_tiles_and_groups(al, long_sets, long_brute, tile_cols, k, cutoff, strands):
    queries, targets = long_sets
    cg = k == 3
    got = al.scan(queries, targets, k=k, cutoff=cutoff, strands=strands, tile_cols=tile_cols, cigar=cg, cigar_m=cg and strands == "both")
    cfg = al.last_config
    assert cfg.startswith("scan: tile=%d " % (tile_cols or A.scan_plan(1, 1)[0])) and "myers-scan bits=2 words/lane=" in cfg, cfg
    if tile_cols == 16:
        groups = int(cfg.split("groups=")[1].split()[0])
        assert groups == sum(max(1, -(-len(t) // 1024)) for t in targets) and groups > len(targets)      # several groups per long target
    want = _expected(long_brute, STRANDS_OF[strands], k, cutoff)
    _same(got, want, NAMES + (("strand",) if strands == "both" else ()), (tile_cols, k, cutoff, strands))
    if cg:
        assert "windows: myers-infix-tb" in cfg, cfg
        _check_cigars(got, queries, targets, strands == "both")


@pytest.mark.gpu
@pytest.mark.parametrize("tile_cols", [16, 64, 0])
def test_ties(al, tile_cols):
    rng = random.Random(9)
    q = _rnd(rng, 40)
    pal = _rc(q[:20]) + q[:20]
    body = list(_rnd(rng, 5000))
    for end in (1040, 1024 + 64 * 16 + 7, 3000, 4999):          # the same exact copy in several tiles and groups
        body[end - 40:end] = q
    t_multi = "".join(body)
    queries = [q, pal, "A" * 70, _rnd(rng, 300)]
    targets = [_rnd(rng, 900), t_multi, t_multi, "A" * 2500, _rnd(rng, 120), pal + _rnd(rng, 50) + pal]
    full = _brute(queries, targets)
    assert full["end_j"][0, 0, 1] == 1040 and full["score"][0, 0, 1] == 0
    assert full["end_j"][2, 0, 3] == 70 and full["score"][2, 0, 3] == 0             # poly-A in poly-A: the first column that has it
    assert len(queries[3]) > len(targets[4])                                        # a read longer than its target
    for strands in ("forward", "both"):
        for k in (1, 5):
            got = al.scan(queries, targets, k=k, strands=strands, tile_cols=tile_cols, cigar=True)
            _same(got, _expected(full, STRANDS_OF[strands], k, None), NAMES + (("strand",) if strands == "both" else ()), (tile_cols, k, strands))
            _check_cigars(got, queries, targets, False)
    got = al.scan(queries, targets, k=4, strands="both", tile_cols=tile_cols)
    assert list(got["target"][0, :2]) == [1, 2]                                     # duplicate targets: the smaller index first
    assert list(got["target"][1, :2]) == [5, 5] and list(got["strand"][1, :2]) == [0, 1]   # its own reverse complement: strand 0 first


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, None])
def test_slices_give_identical_lists(al, long_sets, long_brute, monkeypatch, chunk):
    queries, targets = long_sets
    if chunk is None:
        monkeypatch.delenv("AT_ALLPAIRS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("AT_ALLPAIRS_CHUNK", str(chunk))
    for strands in ("forward", "both"):
        got = al.scan(queries, targets, k=3, strands=strands, tile_cols=64)
        _same(got, _expected(long_brute, STRANDS_OF[strands], 3, None), NAMES + (("strand",) if strands == "both" else ()), (chunk, strands))


@pytest.mark.gpu
@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("cutoff", [None, 12], ids=["all", "cutoff12"])
@pytest.mark.parametrize("k", [1, 3, 64])
def test_scan_equals_search_on_an_infix_handle(al, infix_sets, k, cutoff, strands):
    queries, targets = infix_sets
    ref = A.Aligner()
    try:
        ref.set_scoring(*UNIT)
        ref.set_edit_infix(True)
        want = ref.search("edit", queries, targets, k=k, cutoff=cutoff, strands=strands)
    finally:
        ref.close()
    for tile_cols in (32, 0):
        got = al.scan(queries, targets, k=k, cutoff=cutoff, strands=strands, tile_cols=tile_cols)
        _same(got, want, NAMES + (("strand",) if strands == "both" else ()), (k, cutoff, strands, tile_cols))


@pytest.mark.gpu
def test_settings_neither_matter_nor_change(al, long_sets, long_brute):
    queries, targets = long_sets
    on = A.Aligner()
    try:
        on.set_scoring(*UNIT)
        on.set_edit_infix(True)
        on.set_edit_traceback(True)
        a = al.scan(queries, targets, k=3, strands="both", tile_cols=64, cigar=True)
        assert al.last_config.startswith("scan: "), al.last_config
        b = on.scan(queries, targets, k=3, strands="both", tile_cols=64, cigar=True)
        for name in NAMES + ("strand", "ncigar", "stats", "cigar_off"):
            assert np.array_equal(a[name], b[name]), name
        _same(a, _expected(long_brute, (0, 1), 3, None), NAMES + ("strand",), "settings")
        # the first handle is still global and number-only, the second still infix with op lists
        pair = [(queries[3], targets[5])]
        r = al.align_batch("edit", pair)
        assert "infix" not in al.last_config, al.last_config
        assert int(r["score"][0]) == _global_ref(queries[3].encode(), targets[5].encode())[0] and int(r["end_j"][0]) == len(targets[5]) and "ops" not in r
        r = on.align_batch("edit", pair)
        d, js, ops, _j0 = _infix_ref(queries[3].encode(), targets[5].encode())
        assert (int(r["score"][0]), int(r["end_j"][0]), r["ops"][0]) == (d, js, ops)
    finally:
        on.close()


@pytest.mark.gpu
def test_refusals(al, long_sets, long_brute):
    queries, targets = long_sets
    q, t = queries[:4], targets[4:7]
    two = A.Aligner()
    try:
        two.set_scoring(1, 2, -5, -1, -10)
        with pytest.raises(A.AlignToolsError) as ei:
            two.scan(q, t)
        assert ei.value.code == A.ERR_DOMAIN and "u = 2, not 1" in str(ei.value), ei.value
    finally:
        two.close()
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan(q, t + ["ACGTNACGT" * 30])
    assert ei.value.code == A.ERR_DOMAIN and "ACGT" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan(q + ["ACGTA" * 205], t)
    assert ei.value.code == A.ERR_DOMAIN and "1025 bases, more than 1024" in str(ei.value), ei.value
    for k in (0, 65):
        with pytest.raises(A.AlignToolsError) as ei:
            al.scan(q, t, k=k)
        assert ei.value.code == A.ERR_ARG and "k = %d outside 1..64" % k in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.scan(q, t, tile_cols=24)
    assert ei.value.code == A.ERR_ARG and "tile_cols = 24" in str(ei.value) and "multiple of 16" in str(ei.value), ei.value
    # the handle works afterwards; nt == 0 gives 0 hits
    got = al.scan(queries, targets, k=3, tile_cols=64)
    _same(got, _expected(long_brute, (0,), 3, None), NAMES, "after the refusals")
    got = al.scan(q, [], k=2, cigar=True)
    assert (got["nhits"] == 0).all() and (got["target"] == -1).all() and (got["ncigar"] == 0).all() and (got["stats"] == -1).all()


@pytest.mark.gpu
def test_small_cigar_buffer_and_guard_bytes(al, long_sets):
    queries, targets = long_sets
    qs, ts = [q.encode() for q in queries[5:9]], [t.encode() for t in targets[5:8]]
    k, nq, nt = 2, 4, 3
    full = al.scan(queries[5:9], targets[5:8], k=k, cigar=True, tile_cols=64)
    n = nq * k
    total = int(full["cigar_off"][n])
    assert total > 8

    def pack(seqs):
        lens = np.array([len(x) for x in seqs], dtype=np.int32)
        off = np.concatenate(([0], np.cumsum(lens[:-1]))).astype(np.int64)
        return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy(), off, lens
    qb, qo, ql = pack(qs)
    tb, to, tl = pack(ts)
    G, GUARD = 16, 0x5a5a5a5a
    cap = int(full["cigar_off"][3])                               # room for the first three entries only
    assert 0 < cap < total
    i32 = {name: np.full(n + G, GUARD, dtype=np.int32) for name in ("target", "score", "end_i", "end_j", "state", "ncigar")}
    nhits = np.full(nq + G, GUARD, dtype=np.int32)
    stats = np.full(n * 8 + G, GUARD, dtype=np.int32)
    coff = np.full(n + 1 + G, GUARD, dtype=np.int64)
    words = np.full(cap + G, GUARD, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = al._lib.at_scan(al._h, nq, p(qb), p(qo), p(ql), nt, p(tb), p(to), p(tl), k, 0, 0, A.STRAND_FWD, 64, 0,
                         p(i32["target"]), p(i32["score"]), p(i32["end_i"]), p(i32["end_j"]), p(i32["state"]), None, p(nhits),
                         p(stats), p(i32["ncigar"]), p(coff), p(words), cap)
    assert rc == 0, al._lib.at_last_error(al._h)
    for name in ("target", "score", "end_i", "end_j", "state", "ncigar"):
        assert np.array_equal(i32[name][:n], full[name].reshape(-1)), name
        assert (i32[name][n:] == GUARD).all(), name
    assert np.array_equal(nhits[:nq], full["nhits"]) and (nhits[nq:] == GUARD).all()
    assert np.array_equal(stats[:n * 8], full["stats"].reshape(-1)) and (stats[n * 8:] == GUARD).all()
    assert np.array_equal(coff[:n + 1], full["cigar_off"]) and (coff[n + 1:] == GUARD).all()      # counts and offsets are complete
    flat = np.concatenate([w for row in full["cigar"] for w in row])
    assert np.array_equal(words[:cap], flat[:cap]) and (words[cap:] == GUARD).all()
