"""Edit infix mode (at_set_edit_infix): the best match of a read inside a target -- D(0,j) = 0, score = min over j of D(l1,j), end cell
(l1, j*) with the smallest such j, ops from (l1, j*) to (0, j0).

The expected values come from the restatement below: the rows-of-numpy table of tests/test_edit_align.py with D[0] = 0, np.argmin of
its last row, and the three-way rule of include/aligntools_hip.h.  On the CPU the restatement is anchored to the committed oracle:
its score and j* equal the minimum over all substrings of the oracle's global distance, smallest end first.  On the GPU every pair of
every batch is compared: ops byte for byte, nops, score, end cell and state."""
import ctypes as C
import functools
import itertools
import random

import numpy as np
import pytest

import oracle as O

import aligntools.c_amd as A

UNIT = (1, 1, -5, -1, -10)          # m, u, o, e, j: u = 1 is the only cost the bit-parallel path has
INT32_MIN = -2 ** 31


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def _table(s1, s2, infix):
    a, b = np.frombuffer(s1, dtype=np.uint8), np.frombuffer(s2, dtype=np.uint8)
    l1, l2 = len(a), len(b)
    jj = np.arange(l2 + 1, dtype=np.int32)
    D = np.zeros((l1 + 1, l2 + 1), dtype=np.int32)
    D[0] = 0 if infix else jj
    cand = np.zeros(l2 + 1, dtype=np.int32)
    for i in range(1, l1 + 1):
        cand[0] = i
        cand[1:] = np.minimum(D[i - 1, :-1] + (b != a[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(cand - jj) + jj
    return a, b, D


@functools.lru_cache(maxsize=None)
def _infix_ref(s1, s2):
    """(score, j*, ops END -> START, j0) of two bytes objects by the rule of the header"""
    a, b, D = _table(s1, s2, True)
    l1 = len(a)
    js = int(np.argmin(D[l1]))
    i, j, ops = l1, js, bytearray()
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
    return int(D[l1, js]), js, bytes(ops), j


@functools.lru_cache(maxsize=None)
def _global_ref(s1, s2):
    """(distance, ops END -> START) of the GLOBAL rule (at_set_edit_traceback), for the setting switched off"""
    a, b, D = _table(s1, s2, False)
    i, j, ops = len(a), len(b), bytearray()
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1, j - 1] + (a[i - 1] != b[j - 1]) == D[i, j]:
            ops.append(A.OP_MID)
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1, j] + 1 == D[i, j]:
            ops.append(A.OP_LOW)
            i -= 1
        else:
            ops.append(A.OP_UPP)
            j -= 1
    return int(D[len(a), len(b)]), bytes(ops)


def _cost(ops, s1, s2, end_j):
    """(mismatch columns + gap columns, the cell the list ends in) of a walk from (l1, end_j)"""
    i, j, c = len(s1), end_j, 0
    for op in ops:
        if op == A.OP_MID:
            i, j = i - 1, j - 1
            c += s1[i] != s2[j]
        elif op == A.OP_LOW:
            i, c = i - 1, c + 1
        else:
            assert op == A.OP_UPP
            j, c = j - 1, c + 1
        assert i >= 0 and j >= 0
    return c, (i, j)


def _rand(rng, n, alpha):
    return bytes(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, alpha):
    """s with up to 8 % substitutions and up to two short indel runs"""
    t = bytearray(s)
    for _ in range(rng.randint(0, max(1, len(t) * 8 // 100))):
        if t:
            t[rng.randrange(len(t))] = rng.choice(alpha)
    for _ in range(rng.randint(0, 2)):
        q, run = rng.randrange(len(t) + 1), rng.randint(1, 3)
        if rng.random() < 0.5:
            del t[q:q + run]
        else:
            t[q:q] = _rand(rng, run, alpha)
    return bytes(t)


def _target(rng, a, l2, alpha, related):
    """a target of exactly l2 bases; related: a mutated copy of the read (or the piece of it that fits) planted somewhere in it"""
    if not related or l2 <= 0:
        return _rand(rng, max(l2, 0), alpha)
    piece = _mutate(rng, a, alpha)[:l2]
    at = rng.randint(0, l2 - len(piece))
    return _rand(rng, at, alpha) + piece + _rand(rng, l2 - at - len(piece), alpha)


def _check(res, pairs, ctx="", ops=True):
    for k, (a, b) in enumerate(pairs):
        d, js, ref, _j0 = _infix_ref(a, b)
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]))
        assert got == (d, len(a), js, A.ST_MID), (ctx, k, len(a), len(b), got, (d, js))
        if ops:
            assert int(res["nops"][k]) == len(ref) and res["ops"][k] == ref, (ctx, k, len(a), len(b))
        else:
            assert int(res["nops"][k]) == 0, (ctx, k)


# ---------------------------------------------------------------- CPU

@functools.lru_cache(maxsize=None)
def _oracle_dist(a, b):
    r = O.align(O.EDIT, a, b, u=1)
    assert r["rc"] == 0
    return int(r["score"])


def _small_strings(top):
    return [bytes(t) for n in range(top + 1) for t in itertools.product(b"AC", repeat=n)]


def test_restatement_equals_brute_force_over_substrings():
    """all pairs of {A,C} strings with l1 <= 4, l2 <= 5: score and j* are the minimum over the substrings b[s:e] of the oracle's
    global distance, the smallest e first; the op list costs the score and ends in (0, j0) with lev(a, b[j0:j*]) == score"""
    n = 0
    for a in _small_strings(4):
        for b in _small_strings(5):
            d, js, ops, j0 = _infix_ref(a, b)
            best = min((min(_oracle_dist(a, b[s:e]) for s in range(e + 1)), e) for e in range(len(b) + 1))
            assert (d, js) == best, (a, b)
            assert _cost(ops, a, b, js) == (d, (0, j0)) and len(ops) <= len(a) + len(b), (a, b)
            assert 0 <= j0 <= js and _oracle_dist(a, b[j0:js]) == d, (a, b)
            n += 1
    assert n == 31 * 63


def test_worked_examples_of_the_header():
    M, L = A.OP_MID, A.OP_LOW
    assert _infix_ref(b"ACGT", b"ACGTACGTACGT") == (0, 4, bytes([M, M, M, M]), 0)
    assert _infix_ref(b"ACGTA", b"CG") == (3, 2, bytes([L, L, M, M, L]), 0)
    assert _infix_ref(b"", b"ACG")[:2] == (0, 0) and _infix_ref(b"ACG", b"") == (3, 0, bytes([L, L, L]), 0)


def test_symbol_is_exported_and_listed():
    from aligntools.c_amd import build
    build.build()
    lib = A.load_library()
    assert "at_set_edit_infix" in A.ABI_SYMBOLS
    assert lib.at_set_edit_infix is not None
    assert lib.at_set_edit_infix(None, 1) == A.ERR_ARG
    assert b"at_set_edit_infix" in lib.at_last_error(None)
    assert callable(A.Aligner.set_edit_infix)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    a.set_scoring(*UNIT)
    a.set_edit_traceback(True)
    a.set_edit_infix(True)
    yield a
    a.close()


@pytest.fixture
def one_chunk(monkeypatch):
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")     # (a chunk on a helper handle would keep its own last_config)
    return monkeypatch


def _both(al, pairs, ctx, W=None):
    """the ops form and the number-only form of one batch, each proven to have taken the infix route"""
    res = al.align_batch("edit", pairs, render=False)
    cfg = al.last_config
    assert cfg.startswith("myers-infix-tb bits=2 words/lane=") and "slab=" in cfg and "grid=" in cfg, cfg
    if W:
        assert cfg.startswith("myers-infix-tb bits=2 words/lane=%d " % W), cfg
    _check(res, pairs, ctx)
    num = al.align_batch("edit", pairs, traceback=False)
    cfg = al.last_config
    assert cfg.startswith("myers-infix bits=2 words/lane=") and "ops" not in num, cfg
    if W:
        assert cfg.startswith("myers-infix bits=2 words/lane=%d " % W), cfg
    _check(num, pairs, ctx, ops=False)
    return res


L1S = [1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 256, 257, 512, 513, 1023, 1024]
WORDS = {64: 2, 96: 3, 128: 4, 160: 5, 256: 8, 512: 16, 1024: 32}


def _l2s(l1):
    return [x for x in (1, 15, 16, 17, 31, 32, 33, 48, l1 - 7, l1 + 40) if x > 0]


@pytest.mark.gpu
@pytest.mark.parametrize("l1", L1S)
def test_word_classes(al, one_chunk, l1):
    """a read length at an edge of a word class against every listed target length: related and unrelated pairs over AC (ties
    everywhere) and ACGT; the batch's longest read is l1, so the class is the one l1 selects"""
    rng = random.Random(l1)
    W = WORDS[min(t for t in WORDS if t >= l1)]
    pairs = []
    for l2 in _l2s(l1):
        for alpha in (b"AC", b"ACGT"):
            for related in (True, False):
                a = _rand(rng, l1, alpha)
                pairs.append((a, _target(rng, a, l2, alpha, related)))
    _both(al, pairs, l1, W)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_sizes(al, one_chunk, n):
    """partial wavefronts"""
    rng = random.Random(100 + n)
    pairs = []
    for k in range(n):
        a = _rand(rng, rng.randint(20, 70), b"ACGT")
        pairs.append((a, _target(rng, a, rng.randint(40, 120), b"ACGT", k % 3 != 0)))
    _both(al, pairs, n)


@pytest.mark.gpu
def test_mixed_lengths_in_one_wavefront(al, one_chunk):
    """130 pairs with l1 uniform in 1..160 and l2 uniform in 0..220: the tracking stops at the lane's own l2 and short reads work
    in a wide class"""
    rng = random.Random(2)
    pairs = []
    for k in range(130):
        alpha = b"AC" if k % 2 else b"ACGT"
        a = _rand(rng, rng.randint(1, 160), alpha)
        pairs.append((a, _target(rng, a, rng.randint(0, 220), alpha, k % 3 != 0)))
    pairs[0] = (_rand(rng, 160, b"ACGT"), pairs[0][1])
    res = _both(al, pairs, "mixed", 5)
    for k, (a, b) in enumerate(pairs):
        d, js, ops, j0 = _infix_ref(a, b)
        assert _cost(res["ops"][k], a, b, js) == (d, (0, j0)), k


@pytest.mark.gpu
def test_borders_and_ties(al, one_chunk):
    rng = random.Random(3)
    t = _rand(rng, 90, b"ACGT")
    pairs = [(b"", b"ACGTACG"), (b"GATTACA", b""), (b"", b""), (b"ACGTA", b"CG"), (_rand(rng, 70, b"ACGT"), _rand(rng, 20, b"ACGT")),
             (b"ACGT", b"ACGTACGTACGT"), (t[-33:], t), (t[:33], t), (b"A", b"CCCACCC"), (b"G", b"CCCC"), (b"C", b"C"),
             (b"AAAA", b"AAAAAAAAAAAA"), (b"ACAC", b"CACACACA")]
    res = _both(al, pairs, "borders")
    assert (int(res["score"][5]), int(res["end_j"][5])) == (0, 4)
    assert (int(res["score"][6]), int(res["end_j"][6])) == (0, 90) and (int(res["score"][7]), int(res["end_j"][7])) == (0, 33)
    assert [int(res["score"][k]) for k in range(4)] == [0, 7, 0, 3] and [int(res["end_j"][k]) for k in range(4)] == [0, 0, 0, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65])
def test_device_entry(al, n):
    """the device entry (the processing order of the host entry's ragged batches is covered by the host tests around this one):
    slots in shuffled order with guard bytes between and behind them -- only nops[k] bytes of a slot change; a pair longer than
    max_len1 comes back refused (score INT32_MIN, nops -1) with nothing else written"""
    import torch
    rng = random.Random(60 + n)
    max1, max2 = 90, 120
    pairs = []
    for _ in range(n):
        a = _rand(rng, rng.randint(1, max1), b"ACGT")
        pairs.append((a, _target(rng, a, rng.randint(1, max2), b"ACGT", True)))
    long_k = 5 if n > 5 else -1
    if long_k >= 0:
        pairs[long_k] = (_rand(rng, max1 + 7, b"ACGT"), pairs[long_k][1])
    words, woff1, woff2, len1, len2, bits = A.pack_pairs(pairs)
    assert bits == 2
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("w", words.view(np.int32)), ("o1", woff1), ("o2", woff2), ("l1", len1), ("l2", len2))}
    slot = max1 + 7 + max2 + 9
    perm = list(range(n))
    rng.shuffle(perm)
    ops_off = np.array([16 + perm[k] * slot for k in range(n)], dtype=np.int64)
    d_off = torch.from_numpy(ops_off).to(dev)
    for tb in (True, False):
        ops = torch.full((16 + n * slot + 64,), 0xEE, dtype=torch.uint8, device=dev)
        out = torch.full((5, n), -7, dtype=torch.int32, device=dev)
        al.align_batch_device(A.MODE_EDIT, n, d["w"].data_ptr(), bits, d["o1"].data_ptr(), d["l1"].data_ptr(), d["o2"].data_ptr(),
                              d["l2"].data_ptr(), max1, max2, False, tb, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                              out[3].data_ptr(), ops.data_ptr(), d_off.data_ptr(), out[4].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert al.last_config.startswith("myers-infix-tb bits=2 words/lane=3 " if tb else "myers-infix bits=2 words/lane=3 "), al.last_config
        o = out.cpu().numpy()
        got = ops.cpu().numpy()
        want = np.full(len(got), 0xEE, dtype=np.uint8)
        for k, (a, b) in enumerate(pairs):
            if k == long_k:
                assert [int(o[r][k]) for r in range(5)] == [INT32_MIN, -7, -7, -7, -1], k
                continue
            dist, js, ref, _j0 = _infix_ref(a, b)
            assert [int(o[r][k]) for r in range(5)] == [dist, len(a), js, A.ST_MID, len(ref) if tb else 0], (tb, k)
            if tb:
                want[ops_off[k]:ops_off[k] + len(ref)] = np.frombuffer(ref, dtype=np.uint8)
        assert np.array_equal(got, want), tb


@pytest.mark.gpu
def test_chunked_host_path_equals_the_unchunked(al, monkeypatch):
    """2 x AT_HOST_CHUNK_MIN + 7 ragged pairs (the host entry hands them out in its own order, largest first): the helper handles of
    the chunks inherit the setting, and the results equal those of one chunk"""
    monkeypatch.setenv("AT_HOST_CHUNK_MIN", "1024")
    rng = random.Random(8)
    pairs = []
    for k in range(2 * 1024 + 7):
        a = _rand(rng, rng.randint(20, 40), b"ACGT")
        pairs.append((a, _target(rng, a, rng.randint(30, 70), b"ACGT", k % 4 != 0)))
    res = al.align_batch("edit", pairs, render=False)
    assert "myers-infix-tb" in al.last_config and " x2 chunks" in al.last_config, al.last_config
    _check(res, pairs, "chunked")
    num = al.align_batch("edit", pairs, traceback=False)
    assert al.last_config.startswith("myers-infix bits=2") and " x2 chunks" in al.last_config, al.last_config
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    one = al.align_batch("edit", pairs, render=False)
    assert " chunks" not in al.last_config, al.last_config
    for key in ("score", "end_i", "end_j", "state", "nops"):
        assert np.array_equal(res[key], one[key]), key
    assert res["ops"] == one["ops"]
    assert np.array_equal(num["score"], one["score"]) and np.array_equal(num["end_j"], one["end_j"])


@pytest.mark.gpu
def test_consumers(al, one_chunk):
    """The strings form is the rendering of the ops, the CIGAR form their host CIGAR; START_J is j0 and the counts sum to the score"""
    rng = random.Random(7)
    pairs = [(b"", b"ACG"), (b"ACGT", b"ACGTACGTACGT"), (b"ACGTA", b"CG")]
    while len(pairs) < 90:
        a = _rand(rng, rng.randint(1, 200), b"ACGT")
        pairs.append((a, _target(rng, a, rng.randint(1, 320), b"ACGT", len(pairs) % 5 != 0)))
    ref = al.align_batch("edit", pairs, render=False)
    _check(ref, pairs)
    st = al.align_batch_strings("edit", pairs)
    assert al.last_config.startswith("myers-infix-tb") and "[strings: " in al.last_config, al.last_config
    cg = al.align_batch_cigar("edit", pairs)
    assert al.last_config.startswith("myers-infix-tb") and "[cigar: " in al.last_config, al.last_config
    for k, (a, b) in enumerate(pairs):
        d, js, _ops, j0 = _infix_ref(a, b)
        r1, r2 = al.render(ref["ops"][k], a, len(a), b, js)
        assert (st["r1"][k], st["r2"][k], int(st["nops"][k]), int(st["score"][k]), int(st["end_j"][k])) == (r1, r2, len(r1), d, js), k
        assert r1.replace("-", "").encode() == a and r2.replace("-", "").encode() == b[j0:js], k
        words, stats = A.cigar(ref["ops"][k], a, len(a), b, js)
        assert cg["cigar"][k].tolist() == words.tolist() and cg["stats"][k].tolist() == stats.tolist(), k
        si, sj, eq, ne, ins, dele = (int(x) for x in cg["stats"][k][:6])
        assert (si, sj) == (0, j0) and ne + ins + dele == int(cg["score"][k]) == d and int(cg["end_j"][k]) == js, k
        assert eq + ne + ins == len(a) and eq + ne + dele == js - j0, k


@pytest.mark.gpu
def test_refusals(al, one_chunk):
    """outside the domain: AT_ERR_DOMAIN with the bound named, never the global number"""
    rng = random.Random(5)
    pairs = [(_rand(rng, 40, b"ACGT"), _rand(rng, 64, b"ACGT")) for _ in range(5)]
    for tb in (True, False):
        try:
            al.set_scoring(1, 2, -5, -1, -10)
            with pytest.raises(A.AlignToolsError) as ei:
                al.align_batch("edit", pairs, traceback=tb)
            assert ei.value.code == A.ERR_DOMAIN and "infix" in str(ei.value) and "u = 2" in str(ei.value), ei.value
        finally:
            al.set_scoring(*UNIT)
        with pytest.raises(A.AlignToolsError) as ei:
            al.align_batch("edit", pairs + [(b"ACGTNACGT", b"ACGTACGT")], traceback=tb)
        assert ei.value.code == A.ERR_DOMAIN and "infix" in str(ei.value) and "ACGT" in str(ei.value), ei.value
        with pytest.raises(A.AlignToolsError) as ei:
            al.align_batch("edit", pairs + [(_rand(rng, 1025, b"ACGT"), b"ACGT")], traceback=tb)
        assert ei.value.code == A.ERR_DOMAIN and "infix" in str(ei.value) and "max_len1 = 1025" in str(ei.value), ei.value
        with pytest.raises(A.AlignToolsError) as ei:
            al.align_batch("edit", pairs + [(b"ACGT", _rand(rng, 3793, b"ACGT"))], traceback=tb)
        assert ei.value.code == A.ERR_DOMAIN and "infix" in str(ei.value) and "max_len2 = 3793" in str(ei.value), ei.value
    # all-vs-all in edit mode
    reads = [a for a, _b2 in pairs]
    blob = np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8).copy()
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    off = np.zeros(len(reads), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    npairs = len(reads) * (len(reads) - 1) // 2
    out = [np.zeros(npairs, dtype=np.int32) for _ in range(4)]
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = al._lib.at_align_allpairs(al._h, A.MODE_EDIT, len(reads), ptr(blob), ptr(off), ptr(lens), 0, npairs, 0,
                                   ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), None, None, None)
    assert rc == A.ERR_DOMAIN and b"all-vs-all" in al._lib.at_last_error(al._h), al._lib.at_last_error(al._h)
    with pytest.raises(A.AlignToolsError) as ei:
        al.align_allpairs_stream("edit", blob, off, lens, 0, npairs, 0, lambda *x: None)
    assert ei.value.code == A.ERR_DOMAIN and "all-vs-all" in str(ei.value), ei.value
    # a target of exactly 3 792 bases is inside, and the handle goes on after the refusals
    t = _rand(rng, 3792, b"ACGT")
    edge = [(t[3000:3100], t), (pairs[0][0], t)]
    _both(al, edge + pairs, "after the refusals")


@pytest.mark.gpu
def test_switching_off(al, one_chunk):
    """with the setting off again, the same handle returns the global results on the same pairs"""
    rng = random.Random(9)
    pairs = []
    for k in range(70):
        a = _rand(rng, rng.randint(1, 150), b"ACGT")
        pairs.append((a, _target(rng, a, rng.randint(1, 200), b"ACGT", k % 2 == 0)))
    _both(al, pairs, "on")
    al.set_edit_infix(False)
    try:
        res = al.align_batch("edit", pairs, render=False)
        assert al.last_config.startswith("myers-tb bits=2"), al.last_config
        for k, (a, b) in enumerate(pairs):
            d, ops = _global_ref(a, b)
            got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]), int(res["nops"][k]))
            assert got == (d, len(a), len(b), A.ST_MID, len(ops)) and res["ops"][k] == ops, (k, got)
        num = al.align_batch("edit", pairs, traceback=False)
        assert al.last_config.startswith("myers bits=2"), al.last_config
        assert [int(x) for x in num["score"]] == [_global_ref(a, b)[0] for a, b in pairs]
        assert [int(x) for x in num["end_j"]] == [len(b) for _a, b in pairs]
    finally:
        al.set_edit_infix(True)
    _both(al, pairs[:10], "on again")
