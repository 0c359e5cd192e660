"""at_search / at_search_strands in edit infix mode (at_set_edit_infix): targets rank by where the read fits, not by their length.

40 queries of 30..160 bases against 25 targets of 100..600 bases, some queries planted (as given or reverse-complemented, with
edits), some queries longer than some targets.  The expected lists are the brute-force ranking -- smaller distance first, ties to
the smaller target index, then strand 0 before strand 1 -- of Aligner.align_batch("edit", ...) on all pairs from the same handle,
and those pair results are compared with the restatement of tests/test_edit_infix.py as well."""
import random

import numpy as np
import pytest

import aligntools.c_amd as A
from test_edit_infix import _infix_ref

NAMES = ("target", "score", "end_i", "end_j", "state", "nhits")
STRANDS_OF = {"forward": (0,), "both": (0, 1)}


@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    a.set_scoring(1, 1, -5, -1, -10)
    a.set_edit_infix(True)
    yield a
    a.close()


def _rc(s):
    return A.revcomp(s).decode("latin1")


@pytest.fixture(scope="module")
def sets():
    rng = random.Random(21)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    queries = [rnd(rng.randint(30, 160)) for _ in range(40)]
    queries[0], queries[1] = rnd(30), rnd(160)
    queries[3] = queries[2]                                 # the same query twice
    queries[5] = _rc(queries[4])                            # a query and its reverse complement
    targets = []
    for t in range(25):
        l2 = 100 if t == 0 else 600 if t == 1 else rng.randint(100, 600)
        if t % 5 == 4:
            targets.append(targets[t - 3])                  # a duplicate: ties on every query
            continue
        if t % 2:
            targets.append(rnd(l2))
            continue
        body = list(rng.choice(queries))
        if rng.random() < 0.5:
            body = list(_rc("".join(body)))
        for _ in range(rng.randint(0, 5)):
            body[rng.randrange(len(body))] = rng.choice("ACGT")
        if rng.random() < 0.5:
            del body[rng.randrange(len(body))]
        body = "".join(body)[:l2]
        at = rng.randint(0, l2 - len(body))
        targets.append(rnd(at) + body + rnd(l2 - at - len(body)))
    assert min(len(t) for t in targets) == 100 and max(len(t) for t in targets) == 600
    assert any(len(q) > len(t) for q in queries for t in targets)
    return queries, targets


@pytest.fixture(scope="module")
def brute(al, sets):
    """score / end_i / end_j / state of every (query, strand, target) from align_batch on the same handle: arrays (nq, 2, nt), each
    compared with the restatement once"""
    queries, targets = sets
    nq, nt = len(queries), len(targets)
    seqs = [queries, [_rc(q) for q in queries]]
    idx = [(a, s, b) for a in range(nq) for s in (0, 1) for b in range(nt)]
    res = al.align_batch("edit", [(seqs[s][a], targets[b]) for a, s, b in idx], traceback=False)
    assert al.last_config.startswith("myers-infix bits=2"), al.last_config
    full = {name: np.zeros((nq, 2, nt), dtype=np.int64) for name in ("score", "end_i", "end_j", "state")}
    for n, (a, s, b) in enumerate(idx):
        d, js, _ops, _j0 = _infix_ref(seqs[s][a].encode(), targets[b].encode())
        got = tuple(int(res[name][n]) for name in ("score", "end_i", "end_j", "state"))
        assert got == (d, len(queries[a]), js, A.ST_MID), (a, s, b, got)
        for name, v in zip(("score", "end_i", "end_j", "state"), got):
            full[name][a, s, b] = v
    return full


def _expected(full, strands, k, cutoff):
    nq, _, nt = full["score"].shape
    out = {name: np.full((nq, k), -1 if name in ("target", "strand") else 0, dtype=np.int64)
           for name in ("target", "score", "end_i", "end_j", "state", "strand")}
    nhits = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        # candidates in (target, strand) order, so that a stable sort by distance leaves ties in the rule's order
        cand = [(t, s) for t in range(nt) for s in strands]
        if cutoff is not None:
            cand = [(t, s) for t, s in cand if full["score"][q, s, t] <= cutoff]
        cand.sort(key=lambda ts: full["score"][q, ts[1], ts[0]])
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
        assert np.array_equal(np.asarray(got[name], dtype=np.int64), np.asarray(want[name], dtype=np.int64)), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("cutoff", [None, 12], ids=["all", "cutoff12"])
@pytest.mark.parametrize("k", [1, 3, 64])
def test_search_equals_brute_force(al, sets, brute, k, cutoff, strands):
    queries, targets = sets
    got = al.search("edit", queries, targets, k=k, cutoff=cutoff, strands=strands)
    assert "myers-infix bits=2" in al.last_config and al.last_config.startswith("search: "), al.last_config
    want = _expected(brute, STRANDS_OF[strands], k, cutoff)
    _same(got, want, NAMES + (("strand",) if strands == "both" else ()), (k, cutoff, strands))
    if cutoff is None:
        assert (got["nhits"] == min(k, len(targets) * len(STRANDS_OF[strands]))).all()      # every pair is a candidate, whatever the lengths
    else:
        assert 0 < int(got["nhits"].sum()) < len(queries) * min(k, len(targets) * len(STRANDS_OF[strands]))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_search_slices_give_identical_lists(al, sets, brute, monkeypatch, chunk):
    queries, targets = sets
    monkeypatch.setenv("AT_ALLPAIRS_CHUNK", str(chunk))
    for strands in ("forward", "both"):
        got = al.search("edit", queries, targets, k=3, strands=strands)
        _same(got, _expected(brute, STRANDS_OF[strands], 3, None), NAMES + (("strand",) if strands == "both" else ()), (chunk, strands))


@pytest.mark.gpu
def test_search_outside_the_domain_fails(al, sets):
    queries, targets = sets
    with pytest.raises(A.AlignToolsError) as ei:
        al.search("edit", queries[:3], targets[:3] + ["ACGTNNACGT" * 12])
    assert ei.value.code == A.ERR_DOMAIN and "infix" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.search("edit", queries[:3] + ["ACGT" * 257], targets[:3])
    assert ei.value.code == A.ERR_DOMAIN and "max_len1 = 1028" in str(ei.value), ei.value
