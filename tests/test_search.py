"""at_search / Aligner.search: every query against every target, the best k hits per query, selected on the device.

The GPU tests derive the expected hits from Aligner.align_batch on the explicit N x M pair list (the entry pinned to the
oracle) with a stable numpy sort under the rank rule: higher score first (edit: smaller distance first), ties: smaller
target index first, cut to k, filtered by the cutoff.  Without a GPU only the argument checks run."""
import ctypes as C
import os
import random
import zlib

import numpy as np
import pytest

import aligntools.c_amd as A
import oracle as O

SCORING = (1, -2, -5, -1, -10)
SITES = [7, 30, 31, 60, 95, 140, 300]


@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


def test_search_null_handle_is_arg_error(lib):
    q = np.frombuffer(b"ACGT\0", dtype=np.uint8)
    off = np.zeros(1, dtype=np.int64)
    ln = np.full(1, 4, dtype=np.int32)
    outs = [np.zeros(1, dtype=np.int32) for _ in range(6)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.at_search(None, A.MODE_LOCAL, 1, p(q), p(off), p(ln), 1, p(q), p(off), p(ln), 1, 0, 0, *[p(o) for o in outs])
    assert rc == -1
    assert b"NULL handle" in lib.at_last_error(None)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def al():
    a = A.Aligner(0)
    yield a
    a.close()


def _sets(alphabet, nq=60, nt=300, seed=11):
    rng = random.Random(seed)
    queries = ["".join(rng.choice(alphabet) for _ in range(rng.randint(20, 200))) for _ in range(nq)]
    targets = []
    for t in range(nt):
        if t >= 10 and rng.random() < 0.1:
            targets.append(targets[rng.randrange(t)])                      # duplicates force ties
        elif rng.random() < 0.3:
            q = rng.choice(queries)                                        # a target that contains a query (with edits)
            a = rng.randint(0, 200)
            body = list(q)
            for _ in range(rng.randint(0, 6)):
                body[rng.randrange(len(body))] = rng.choice(alphabet)
            targets.append("".join(rng.choice(alphabet) for _ in range(a)) + "".join(body) + "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 100))))
        else:
            targets.append("".join(rng.choice(alphabet) for _ in range(rng.randint(10, 600))))
    return queries, targets


def _brute(al, mode, queries, targets):
    """score / end_i / end_j / state of every (query, target) pair from align_batch, as (nq, nt) arrays (fit: invalid = None)."""
    nq, nt = len(queries), len(targets)
    valid = np.ones((nq, nt), dtype=bool)
    if mode == "fit":
        valid = np.array([[len(q) <= len(t) for t in targets] for q in queries])
    idx = np.argwhere(valid)
    res = al.align_batch(mode, [(queries[a], targets[b]) for a, b in idx], traceback=False)
    full = {}
    for name in ("score", "end_i", "end_j", "state"):
        m = np.zeros((nq, nt), dtype=np.int64)
        m[idx[:, 0], idx[:, 1]] = res[name]
        full[name] = m
    return valid, full


def _expected(mode, valid, full, k, cutoff):
    nq, nt = valid.shape
    out = {name: np.full((nq, k), -1 if name == "target" else 0, dtype=np.int64) for name in ("target", "score", "end_i", "end_j", "state")}
    nhits = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        t = np.flatnonzero(valid[q])
        s = full["score"][q, t]
        if cutoff is not None:
            keep = s <= cutoff if mode == "edit" else s >= cutoff
            t, s = t[keep], s[keep]
        rank = s if mode == "edit" else -s
        order = np.argsort(rank, kind="stable")[:k]                        # t ascending, stable: ties keep the smaller index
        hit = t[order]
        nhits[q] = len(hit)
        out["target"][q, :len(hit)] = hit
        for name in ("score", "end_i", "end_j", "state"):
            out[name][q, :len(hit)] = full[name][q, hit]
    out["nhits"] = nhits
    return out


def _same(got, want, what):
    for name in ("target", "score", "end_i", "end_j", "state", "nhits"):
        assert np.array_equal(np.asarray(got[name], dtype=np.int64), want[name]), (what, name)


def _cutoffs(mode, full, valid):
    s = full["score"][valid]
    return [None, int(np.percentile(s, 40 if mode == "edit" else 60))]


CASES = [("global", False, 1), ("local", False, 1), ("fit", False, 1), ("fit", True, 1), ("overlap", False, 1), ("edit", False, -2),
         ("edit", False, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTN", "ACDEFGHIKLMNPQRSTVWY"], ids=["acgt", "with-N", "protein"])
@pytest.mark.parametrize("mode,jump,u", CASES, ids=["global", "local", "fit", "fit-s", "overlap", "edit", "edit-u1"])
def test_search_equals_brute_force(al, mode, jump, u, alphabet):
    queries, targets = _sets(alphabet, seed=zlib.crc32(repr((mode, jump, u, alphabet)).encode()))
    m, _, o, e, j = SCORING
    al.set_scoring(m, u, o, e, j, jump, SITES if jump else None)
    valid, full = _brute(al, mode, queries, targets)
    for cutoff in _cutoffs(mode, full, valid):
        for k in (1, 5, 64):
            got = al.search(mode, queries, targets, k=k, cutoff=cutoff)
            _same(got, _expected(mode, valid, full, k, cutoff), (mode, jump, u, alphabet, k, cutoff))
    assert al.last_config.startswith("search: ") and ", k=64; " in al.last_config
    # a sample of hits straight against the oracle
    got = al.search(mode, queries, targets, k=3)
    rng = random.Random(3)
    for q in rng.sample(range(len(queries)), 12):
        for h in range(int(got["nhits"][q])):
            t = int(got["target"][q, h])
            r = O.align(O.MODE_NAMES[mode], queries[q], targets[t], m, u, o, e, j, jump, SITES if jump else None)
            want = (r["score"],) if mode == "edit" else (r["score"], r["end_i"], r["end_j"], r["state"])
            have = tuple(int(got[n][q, h]) for n in ("score", "end_i", "end_j", "state"))[:len(want)]
            assert have == want, (mode, q, t)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,jump", [("local", False), ("fit", True), ("edit", False)])
def test_search_slice_independent(al, mode, jump):
    queries, targets = _sets("ACGT", nq=16, nt=70, seed=5)
    al.set_scoring(1, -2, -5, -1, -10, jump, SITES if jump else None)
    old = os.environ.pop("AT_ALLPAIRS_CHUNK", None)
    try:
        base = al.search(mode, queries, targets, k=7)
        for chunk in ("1", "7", "4096"):
            os.environ["AT_ALLPAIRS_CHUNK"] = chunk
            got = al.search(mode, queries, targets, k=7)
            if chunk == "1":
                assert ", k=7; " in al.last_config and " 0 slices" not in al.last_config
            _same(got, {n: np.asarray(v, dtype=np.int64) for n, v in base.items()}, chunk)
    finally:
        os.environ.pop("AT_ALLPAIRS_CHUNK", None)
        if old is not None:
            os.environ["AT_ALLPAIRS_CHUNK"] = old


@pytest.mark.gpu
def test_search_routes_uniform_blocks_to_packed_kernels(al):
    """1 000 queries of 150 x 200 targets of 150, local: one block with the uniform-shape promise -- the packed kernel
    configuration a uniform at_align_batch_device batch of the same 200 000 pairs gets -- and the hits of align_batch."""
    import torch
    rng = random.Random(17)
    queries = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(1000)]
    targets = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(200)]
    for t in range(0, 200, 4):                                             # some targets that share a stretch with a query
        q = queries[rng.randrange(1000)]
        a = rng.randint(0, 100)
        targets[t] = (targets[t][:a] + q[a:a + 50] + targets[t][a + 50:])[:150]
    al.set_scoring(*SCORING)
    got = al.search("local", queries, targets, k=4)
    cfg = al.last_config
    assert cfg.startswith("search: 1 blocks, 1 slices, k=4; "), cfg
    sweep_cfg = cfg.split("; ", 1)[1]
    pairs = [(q, t) for q in queries for t in targets]
    n = len(pairs)
    words, woff1, woff2, len1, len2, bits = A.pack_pairs([(a.encode(), b.encode()) for a, b in pairs])
    dev = torch.device("cuda", 0)
    tt = lambda x: torch.from_numpy(x).to(dev)
    d_words, d_woff1, d_woff2, d_len1, d_len2 = tt(words.view(np.int32)), tt(woff1), tt(woff2), tt(len1), tt(len2)
    d_res = torch.zeros((4, n), dtype=torch.int32, device=dev)
    al.align_batch_device(A.MODE_LOCAL, n, d_words.data_ptr(), bits, d_woff1.data_ptr(), d_len1.data_ptr(), d_woff2.data_ptr(),
                          d_len2.data_ptr(), 150, 150, True, False, d_res[0].data_ptr(), d_res[1].data_ptr(), d_res[2].data_ptr(),
                          d_res[3].data_ptr(), 0, 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert "packed16" in sweep_cfg and sweep_cfg == al.last_config, (sweep_cfg, al.last_config)
    res = al.align_batch("local", pairs, traceback=False)
    full = {name: np.asarray(res[name], dtype=np.int64).reshape(1000, 200) for name in ("score", "end_i", "end_j", "state")}
    assert np.array_equal(d_res[0].cpu().numpy().reshape(1000, 200), full["score"])
    _same(got, _expected("local", np.ones((1000, 200), dtype=bool), full, 4, None), "routing")


@pytest.mark.gpu
def test_search_fit_skips_shorter_targets(al):
    rng = random.Random(29)
    queries = ["".join(rng.choice("ACGT") for _ in range(L)) for L in (30, 80, 120, 200, 250)]
    targets = ["".join(rng.choice("ACGT") for _ in range(L)) for L in (40, 100, 60, 220, 90, 130, 20, 210)]
    al.set_scoring(*SCORING)
    got = al.search("fit", queries, targets, k=8)
    for q, s in enumerate(queries):
        ok = [t for t in range(len(targets)) if len(targets[t]) >= len(s)]
        assert int(got["nhits"][q]) == len(ok), q
        hits = [int(t) for t in got["target"][q, :int(got["nhits"][q])]]
        assert sorted(hits) == ok and all(len(targets[t]) >= len(s) for t in hits)
        assert (got["target"][q, len(ok):] == -1).all()
    # no target is long enough for the last query; none at all: every query has 0 hits
    assert int(got["nhits"][4]) == 0
    none = al.search("fit", queries, [], k=3)
    assert (none["nhits"] == 0).all() and (none["target"] == -1).all()
    with pytest.raises(A.AlignToolsError) as ei:
        al.search("local", queries, targets, k=65)
    assert ei.value.code == -1
    with pytest.raises(A.AlignToolsError) as ei:
        al.search("local", queries + [""], targets, k=1)
    assert ei.value.code == -4
