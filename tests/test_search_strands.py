"""at_search_strands / Aligner.search(strands=...): the search on the reverse-complemented queries, or on both strands.

Expected hits come from Aligner.align_batch (the entry pinned to the oracle) on the explicit pair list built from
revcomp()-ed queries, stable-sorted under the rank rule: better score first (edit: smaller distance), ties to the smaller
target index, then strand 0 before strand 1; cut to k, filtered by the cutoff.  Without a GPU only argument checks run."""
import ctypes as C
import os
import random
import zlib

import numpy as np
import pytest

import aligntools.c_amd as A

SCORING = (1, -2, -5, -1, -10)
SITES = [7, 30, 31, 60, 95, 140, 300]
NAMES = ("target", "score", "end_i", "end_j", "state", "strand", "nhits")
STRANDS_OF = {"forward": (0,), "reverse": (1,), "both": (0, 1)}


@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_search_strands_null_handle_is_arg_error(lib):
    q = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off = np.zeros(1, dtype=np.int64)
    ln = np.full(1, 4, dtype=np.int32)
    outs = [np.zeros(1, dtype=np.int32) for _ in range(7)]
    rc = lib.at_search_strands(None, A.MODE_LOCAL, 1, _p(q), _p(off), _p(ln), 1, _p(q), _p(off), _p(ln), 1, 0, 0, A.STRAND_BOTH,
                               *[_p(o) for o in outs])
    assert rc == -1
    assert b"NULL handle" in lib.at_last_error(None)


def test_search_rejects_unknown_strands_word(lib):
    with pytest.raises(ValueError):
        A.Aligner.search(None, "local", ["ACGT"], ["ACGT"], strands="minus")


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def al():
    a = A.Aligner(0)
    yield a
    a.close()


def _rc(s):
    return A.revcomp(s).decode("latin1")


def _sets(alphabet, nq=40, nt=150, seed=11):
    """Queries of 20..200; targets: random, duplicates (ties), and ones that contain a query or its reverse complement with edits."""
    rng = random.Random(seed)
    rnd = lambda n: "".join(rng.choice(alphabet) for _ in range(n))
    queries = [rnd(rng.randint(20, 200)) for _ in range(nq)]
    queries[3] = queries[2]                                                # the same query twice
    queries[5] = _rc(queries[4])                                           # a query and its reverse complement
    targets = []
    for t in range(nt):
        x = rng.random()
        if t >= 10 and x < 0.1:
            targets.append(targets[rng.randrange(t)])
        elif x < 0.5:
            q = rng.choice(queries)
            if rng.random() < 0.5:
                q = _rc(q)
            body = list(q)
            for _ in range(rng.randint(0, 6)):
                body[rng.randrange(len(body))] = rng.choice(alphabet)
            targets.append(rnd(rng.randint(0, 200)) + "".join(body) + rnd(rng.randint(0, 100)))
        else:
            targets.append(rnd(rng.randint(10, 600)))
    return queries, targets


def _brute(al, mode, queries, targets, strands):
    """score / end_i / end_j / state of every (query, strand, target) from align_batch: arrays (nq, 2, nt); valid marks candidates."""
    nq, nt = len(queries), len(targets)
    valid = np.zeros((nq, 2, nt), dtype=bool)
    for s in strands:
        valid[:, s, :] = True
    if mode == "fit":
        valid &= np.array([[len(q) <= len(t) for t in targets] for q in queries])[:, None, :]
    seqs = [queries, [_rc(q) for q in queries]]
    idx = np.argwhere(valid)
    res = al.align_batch(mode, [(seqs[s][a], targets[b]) for a, s, b in idx], traceback=False)
    full = {}
    for name in ("score", "end_i", "end_j", "state"):
        m = np.zeros((nq, 2, nt), dtype=np.int64)
        m[idx[:, 0], idx[:, 1], idx[:, 2]] = res[name]
        full[name] = m
    return valid, full


def _expected(mode, valid, full, k, cutoff):
    nq, _, nt = valid.shape
    out = {name: np.full((nq, k), -1 if name in ("target", "strand") else 0, dtype=np.int64)
           for name in ("target", "score", "end_i", "end_j", "state", "strand")}
    nhits = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        # candidates in (target, strand) order, so that a stable sort by score leaves ties in the rule's order
        t, s = np.nonzero(valid[q].T)
        sc = full["score"][q, s, t]
        if cutoff is not None:
            keep = sc <= cutoff if mode == "edit" else sc >= cutoff
            t, s, sc = t[keep], s[keep], sc[keep]
        order = np.argsort(sc if mode == "edit" else -sc, kind="stable")[:k]
        t, s = t[order], s[order]
        nhits[q] = len(t)
        out["target"][q, :len(t)] = t
        out["strand"][q, :len(t)] = s
        for name in ("score", "end_i", "end_j", "state"):
            out[name][q, :len(t)] = full[name][q, s, t]
    out["nhits"] = nhits
    return out


def _same(got, want, what):
    for name in NAMES:
        assert np.array_equal(np.asarray(got[name], dtype=np.int64), np.asarray(want[name], dtype=np.int64)), (what, name)


CASES = [("global", False), ("local", False), ("fit", False), ("fit", True), ("overlap", False), ("edit", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTNRYacgt"], ids=["acgt", "8bit"])
@pytest.mark.parametrize("mode,jump", CASES, ids=["global", "local", "fit", "fit-s", "overlap", "edit"])
def test_search_strands_equals_brute_force(al, mode, jump, alphabet):
    queries, targets = _sets(alphabet, seed=zlib.crc32(repr((mode, jump, alphabet)).encode()))
    m, u, o, e, j = SCORING
    al.set_scoring(m, u, o, e, j, jump, SITES if jump else None)
    for strands in ("reverse", "both"):
        valid, full = _brute(al, mode, queries, targets, STRANDS_OF[strands])
        sc = full["score"][valid]
        for cutoff in (None, int(np.percentile(sc, 40 if mode == "edit" else 60))):
            for k in (1, 3, 64):
                got = al.search(mode, queries, targets, k=k, cutoff=cutoff, strands=strands)
                _same(got, _expected(mode, valid, full, k, cutoff), (mode, jump, alphabet, strands, k, cutoff))
        assert al.last_config.startswith("search: ")
        assert (", k=64, strands=%s; " % ("rev" if strands == "reverse" else "both")) in al.last_config


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["local", "fit", "edit"])
def test_forward_through_search_strands_equals_search(al, lib, mode):
    queries, targets = _sets("ACGT", nq=20, nt=60, seed=7)
    al.set_scoring(*SCORING)
    k = 5
    want = al.search(mode, queries, targets, k=k, cutoff=None)
    cfg = al.last_config
    assert ", k=5; " in cfg and "strands" not in cfg
    assert "strand" not in want and sorted(want) == ["end_i", "end_j", "nhits", "score", "state", "target"]
    nq, nt = len(queries), len(targets)

    def pack(seqs):
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        off = np.zeros(len(seqs), dtype=np.int64)
        off[1:] = np.cumsum(lens[:-1])
        return np.frombuffer("".join(seqs).encode() + b"\0", dtype=np.uint8).copy(), off, lens
    qb, qo, ql = pack(queries)
    tb, to, tl = pack(targets)
    outs = [np.full((nq, k), 77, dtype=np.int32) for _ in range(6)]
    nh = np.zeros(nq, dtype=np.int32)
    rc = lib.at_search_strands(al._h, A.MODES[mode], nq, _p(qb), _p(qo), _p(ql), nt, _p(tb), _p(to), _p(tl), k, 0, 0, A.STRAND_FWD,
                               *[_p(o) for o in outs], _p(nh))
    assert rc == 0 and al.last_config == cfg
    for name, o in zip(("target", "score", "end_i", "end_j", "state"), outs):
        assert np.array_equal(o, want[name]), name
    assert np.array_equal(nh, want["nhits"])
    assert np.array_equal(outs[5], np.where(want["target"] >= 0, 0, -1))
    # and without a strand array, as at_search calls it
    outs2 = [np.zeros((nq, k), dtype=np.int32) for _ in range(5)]
    rc = lib.at_search_strands(al._h, A.MODES[mode], nq, _p(qb), _p(qo), _p(ql), nt, _p(tb), _p(to), _p(tl), k, 0, 0, A.STRAND_FWD,
                               *[_p(o) for o in outs2], None, _p(nh))
    assert rc == 0 and np.array_equal(outs2[0], want["target"]) and np.array_equal(outs2[1], want["score"])


@pytest.mark.gpu
def test_search_strands_argument_checks(al, lib):
    """strands outside 1..3, and the read-count limits of a reverse strand, are refused from the counts alone: no array is read."""
    for strands in (0, 4, -1):
        rc = lib.at_search_strands(al._h, A.MODE_LOCAL, 1, None, None, None, 1, None, None, None, 1, 0, 0, strands, *([None] * 7))
        assert rc == -1 and b"strands" in lib.at_last_error(al._h)
    for nq, nt, strands in [(1, 1 << 30, A.STRAND_BOTH), (1, 1 << 30, A.STRAND_REV), (1 << 30, 1, A.STRAND_BOTH), ((1 << 30) - 1, 2, A.STRAND_REV)]:
        rc = lib.at_search_strands(al._h, A.MODE_LOCAL, nq, None, None, None, nt, None, None, None, 1, 0, 0, strands, *([None] * 7))
        assert rc == -1 and b"reverse strand" in lib.at_last_error(al._h), (nq, nt, strands)
    # a reverse strand needs somewhere to report it
    q = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off = np.zeros(1, dtype=np.int64)
    ln = np.full(1, 4, dtype=np.int32)
    outs = [np.zeros(1, dtype=np.int32) for _ in range(5)]
    rc = lib.at_search_strands(al._h, A.MODE_LOCAL, 1, _p(q), _p(off), _p(ln), 1, _p(q), _p(off), _p(ln), 1, 0, 0, A.STRAND_BOTH,
                               *[_p(o) for o in outs], None, _p(ln))
    assert rc == -1
    with pytest.raises(A.AlignToolsError) as ei:
        al.search("local", ["ACGT", ""], ["ACGT"], strands="both")
    assert ei.value.code == -4
    none = al.search("local", ["ACGT"], [], k=2, strands="both")
    assert (none["nhits"] == 0).all() and (none["target"] == -1).all() and (none["strand"] == -1).all()
    assert al.last_config == "search: 0 blocks, 0 slices, k=2, strands=both; "


def _planted():
    rng = random.Random(5)
    targets = ["".join(rng.choice("ACGT") for _ in range(rng.randint(150, 300))) for _ in range(40)]
    queries, truth = [], []
    for q in range(60):
        t = rng.randrange(40)
        n = rng.randint(40, 80)
        a = rng.randint(0, len(targets[t]) - n)
        w = list(targets[t][a:a + n])
        for pos in rng.sample(range(n), 3):
            w[pos] = rng.choice([c for c in "ACGT" if c != w[pos]])
        w = "".join(w)
        strand = q & 1
        queries.append(_rc(w) if strand else w)
        truth.append((t, strand))
    return queries, targets, truth


@pytest.mark.gpu
def test_planted_hits_are_found_on_their_strand(al):
    """Every second query is the reverse complement of a window of its target: the rank-1 hit must be the planted (target, strand).
    A search that ignored or mislabelled the reverse strand would miss 30 of the 60."""
    queries, targets, truth = _planted()
    assert sum(1 for _, s in truth if s == 0) == 30 and sum(1 for _, s in truth if s == 1) == 30
    al.set_scoring(*SCORING)
    got = al.search("local", queries, targets, k=1, strands="both")
    assert (got["nhits"] == 1).all()
    for q, (t, s) in enumerate(truth):
        assert (int(got["target"][q, 0]), int(got["strand"][q, 0])) == (t, s), q
    # one strand alone finds its own half, and scores the other half lower
    fwd = al.search("local", queries, targets, k=1)
    rev = al.search("local", queries, targets, k=1, strands="reverse")
    assert (rev["strand"][:, 0] == 1).all()
    for q, (t, s) in enumerate(truth):
        mine, other = (rev, fwd) if s else (fwd, rev)
        assert int(mine["target"][q, 0]) == t and int(mine["score"][q, 0]) == int(got["score"][q, 0])
        assert int(other["score"][q, 0]) < int(got["score"][q, 0])


@pytest.mark.gpu
def test_palindromes_hit_twice_per_target(al):
    rng = random.Random(9)
    queries = ["ACGT" * 10, "GAATTC", "AATT" * 10]
    for q in queries:
        assert _rc(q) == q
    targets = ["".join(rng.choice("ACGT") for _ in range(rng.randint(60, 120))) for _ in range(6)]
    targets[2] = targets[2][:20] + queries[0] + targets[2][20:]
    al.set_scoring(*SCORING)
    for mode in ("local", "fit", "edit"):
        got = al.search(mode, queries, targets, k=4, strands="both")
        assert (got["nhits"] == 4).all()
        for q in range(len(queries)):
            for h in (0, 2):
                assert int(got["target"][q, h]) == int(got["target"][q, h + 1])
                assert (int(got["strand"][q, h]), int(got["strand"][q, h + 1])) == (0, 1)
                for name in ("score", "end_i", "end_j", "state"):
                    assert int(got[name][q, h]) == int(got[name][q, h + 1]), (mode, q, h, name)
            assert int(got["target"][q, 0]) != int(got["target"][q, 2])
    got = al.search("local", queries, targets, k=4, strands="both")
    assert int(got["target"][0, 0]) == 2 and int(got["score"][0, 0]) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("mode,jump", [("local", False), ("fit", True), ("edit", False)])
def test_search_strands_slice_independent(al, mode, jump):
    """Slices of 1 pair put a boundary everywhere, between the two strands of a query too; 7 cuts query groups unevenly."""
    queries, targets = _sets("ACGT", nq=16, nt=70, seed=5)
    queries[7] = queries[6][:len(queries[6])]                                # two queries of one length: a block of four entries
    queries[8] = _rc(queries[6])
    al.set_scoring(1, -2, -5, -1, -10, jump, SITES if jump else None)
    old = os.environ.pop("AT_ALLPAIRS_CHUNK", None)
    try:
        base = al.search(mode, queries, targets, k=7, strands="both")
        valid, full = _brute(al, mode, queries, targets, (0, 1))
        _same(base, _expected(mode, valid, full, 7, None), "base")
        for chunk in ("1", "7", "4096"):
            os.environ["AT_ALLPAIRS_CHUNK"] = chunk
            got = al.search(mode, queries, targets, k=7, strands="both")
            if chunk == "1":
                assert ", k=7, strands=both; " in al.last_config and " 0 slices" not in al.last_config
            _same(got, base, chunk)
    finally:
        os.environ.pop("AT_ALLPAIRS_CHUNK", None)
        if old is not None:
            os.environ["AT_ALLPAIRS_CHUNK"] = old


@pytest.mark.gpu
def test_both_strands_keep_uniform_blocks_on_packed_kernels(al):
    rng = random.Random(17)
    queries = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(600)]
    targets = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(200)]
    for t in range(0, 200, 4):
        q = queries[rng.randrange(600)]
        if t & 4:
            q = _rc(q)
        a = rng.randint(0, 100)
        targets[t] = (targets[t][:a] + q[a:a + 50] + targets[t][a + 50:])[:150]
    al.set_scoring(*SCORING)
    got = al.search("local", queries, targets, k=4, strands="both")
    cfg = al.last_config
    assert cfg.startswith("search: 1 blocks, 1 slices, k=4, strands=both; "), cfg
    assert "packed16" in cfg.split("; ", 1)[1], cfg
    valid, full = _brute(al, "local", queries, targets, (0, 1))
    _same(got, _expected("local", valid, full, 4, None), "routing")
    assert (got["strand"] == 1).any() and (got["strand"] == 0).any()
