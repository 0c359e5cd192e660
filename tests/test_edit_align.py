"""Edit alignments (at_set_edit_traceback): the alignment behind the number `edit -u 1` returns, on the bit-parallel path.

The expected values come from the restatement below: edit_dist's table with u = 1, one numpy row at a time (the dependency on the
left neighbour is a running minimum of cand - j), then the three-way rule of include/aligntools_hip.h from (l1, l2) to (0, 0).
Every pair of every batch is compared: ops byte for byte, nops, score, end cell and state."""
import ctypes as C
import functools
import random
import re

import numpy as np
import pytest

import oracle as O

import aligntools.c_amd as A

UNIT = (1, 1, -5, -1, -10)          # m, u, o, e, j: u = 1 is the only cost the bit-parallel path has
NOMEM = -6
INT32_MIN = -2 ** 31


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


@functools.lru_cache(maxsize=None)
def _edit_ref(s1, s2):
    """(distance, ops END -> START) of two bytes objects by the rule of the header"""
    a, b = np.frombuffer(s1, dtype=np.uint8), np.frombuffer(s2, dtype=np.uint8)
    l1, l2 = len(a), len(b)
    jj = np.arange(l2 + 1, dtype=np.int32)
    D = np.zeros((l1 + 1, l2 + 1), dtype=np.int32)
    D[0] = jj
    cand = np.zeros(l2 + 1, dtype=np.int32)
    for i in range(1, l1 + 1):
        cand[0] = i
        cand[1:] = np.minimum(D[i - 1, :-1] + (b != a[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(cand - jj) + jj
    i, j, ops = l1, l2, bytearray()
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
    return int(D[l1, l2]), bytes(ops)


def _cost(ops, s1, s2):
    """(mismatch columns + gap columns, the cell the list ends in)"""
    i, j, c = len(s1), len(s2), 0
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


def _related(rng, s1, l2, alpha):
    """s1 with up to 8 % substitutions and short indel runs, cut or padded to l2 bases"""
    t = bytearray(s1)
    for _ in range(rng.randint(0, max(1, len(t) * 8 // 100))):
        if t:
            t[rng.randrange(len(t))] = rng.choice(alpha)
    for _ in range(rng.randint(1, 3)):
        q, run = rng.randrange(len(t) + 1), rng.randint(1, 4)
        if rng.random() < 0.5:
            del t[q:q + run]
        else:
            t[q:q] = _rand(rng, run, alpha)
    t = t[:l2]
    return bytes(t) + _rand(rng, l2 - len(t), alpha)


def _check(res, pairs, ctx=""):
    assert len(res["ops"]) == len(pairs)
    for k, (a, b) in enumerate(pairs):
        d, ops = _edit_ref(a, b)
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]), int(res["nops"][k]))
        assert got == (d, len(a), len(b), A.ST_MID, len(ops)), (ctx, k, len(a), len(b), got)
        assert res["ops"][k] == ops, (ctx, k, len(a), len(b))


# ---------------------------------------------------------------- CPU

def test_restatement_equals_the_oracle_and_its_ops_cost_the_distance():
    rng = random.Random(1)
    n = 0
    for alpha in (b"AC", b"ACGT"):
        for _ in range(200):
            l1, l2 = rng.choice([0, 0, 1, 2, 5, 17, 33, 70]), rng.choice([0, 1, 3, 16, 40, 71])
            a = _rand(rng, l1, alpha)
            b = _related(rng, a, l2, alpha) if rng.random() < 0.5 else _rand(rng, l2, alpha)
            d, ops = _edit_ref(a, b)
            r = O.align(O.EDIT, a, b, u=1)
            assert r["rc"] == 0 and r["score"] == d, (a, b)
            assert _cost(ops, a, b) == (d, (0, 0)) and len(ops) <= l1 + l2
            n += 1
    assert n == 400


def test_symbol_is_exported_and_listed():
    from aligntools.c_amd import build
    build.build()
    lib = A.load_library()
    assert "at_set_edit_traceback" in A.ABI_SYMBOLS
    assert lib.at_set_edit_traceback is not None
    assert lib.at_set_edit_traceback(None, 1) == A.ERR_ARG
    assert b"at_set_edit_traceback" in lib.at_last_error(None)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    a.set_scoring(*UNIT)
    a.set_edit_traceback(True)
    yield a
    a.close()


@pytest.fixture
def one_chunk(monkeypatch):
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")     # (a chunk on a helper handle would keep its own last_config)
    return monkeypatch


CLASSES = [(2, [1, 2, 31, 32, 33, 63, 64]), (3, [65, 96]), (4, [97, 128]), (5, [129, 160]), (8, [161, 255, 256]),
           (16, [257, 511, 512]), (32, [513, 1023, 1024])]


@pytest.mark.gpu
@pytest.mark.parametrize("W,edges", CLASSES, ids=["W%d" % w for w, _ in CLASSES])
def test_word_classes(al, one_chunk, W, edges):
    """67 pairs (a wavefront and three) at the edges of every word class: a third identical, a third related, a third unrelated over
    {A,C}, where ties are everywhere"""
    rng = random.Random(W)
    pairs = []
    for k in range(67):
        l1 = edges[-1] if k == 0 else rng.choice(edges)
        near = [x for x in range(l1 - 3, l1 + 4) if x >= 0]
        a = _rand(rng, l1, b"AC")
        if k % 3 == 0:
            b = a
        elif k % 3 == 1:
            b = _related(rng, a, rng.choice(near), b"AC")
        else:
            b = _rand(rng, rng.choice([0, 1, 15, 16, 17, 31, 32, 33, 2 * l1] + near), b"AC")
        pairs.append((a, b))
    res = al.align_batch("edit", pairs, render=False)
    cfg = al.last_config
    assert cfg.startswith("myers-tb bits=2 words/lane=%d " % W) and "slab=" in cfg and "grid=" in cfg, cfg
    _check(res, pairs, W)
    al.set_edit_traceback(False)
    try:
        plain = al.align_batch("edit", pairs)
        assert "ops" not in plain and al.last_config.startswith("myers bits=2"), al.last_config
    finally:
        al.set_edit_traceback(True)
    assert np.array_equal(plain["score"], res["score"])


@pytest.mark.gpu
def test_ragged_batch(al, one_chunk):
    """130 pairs of 1..300 x 1..300 bases: short and long walks share a wavefront; and the three empty shapes"""
    rng = random.Random(2)
    pairs = [(b"", b""), (b"", b"ACGTACG"), (b"GATTACA", b"")]
    while len(pairs) < 130:
        a = _rand(rng, rng.randint(1, 300), b"ACGT")
        l2 = rng.randint(1, 300)
        pairs.append((a, _related(rng, a, l2, b"ACGT") if rng.random() < 0.5 else _rand(rng, l2, b"AC")))
    rng.shuffle(pairs)
    res = al.align_batch("edit", pairs)
    assert "myers-tb" in al.last_config, al.last_config
    _check(res, pairs)
    for k, (a, b) in enumerate(pairs):
        assert res["r1"][k].replace("-", "").encode() == a and res["r2"][k].replace("-", "").encode() == b, k


@pytest.mark.gpu
def test_slab_reuse_and_an_item_above_the_cap(al, one_chunk):
    """AT_WS_CAP_MB=1: 150 x 150 needs 150 * 5 * 512 slab bytes per wavefront, so two wavefronts work through eight items; an item of
    1024 x 100 (1.6 MB) is refused with AT_ERR_NOMEM and the handle goes on"""
    one_chunk.setenv("AT_WS_CAP_MB", "1")
    rng = random.Random(3)
    pairs = []
    for _ in range(64 * 7 + 5):
        a = _rand(rng, 150, b"ACGT")
        pairs.append((a, _related(rng, a, 150, b"ACGT")))
    res = al.align_batch("edit", pairs, render=False)
    cfg = al.last_config
    assert "words/lane=5 " in cfg and "slab=384000B" in cfg and re.search(r"grid=2\b", cfg), cfg
    _check(res, pairs)
    big = [(_rand(rng, 1024, b"ACGT"), _rand(rng, 100, b"ACGT"))]
    with pytest.raises(A.AlignToolsError) as ei:
        al.align_batch("edit", big)
    assert ei.value.code == NOMEM and "workspace bytes" in str(ei.value), ei.value
    res = al.align_batch("edit", pairs[:70], render=False)
    _check(res, pairs[:70], "after the refusal")


@pytest.mark.gpu
def test_long_second_sequence(al, one_chunk):
    """3 792 bases are what 64 LDS windows hold; one more is outside the domain"""
    rng = random.Random(4)
    pairs = []
    for _ in range(3):
        a = _rand(rng, 100, b"ACGT")
        t = _rand(rng, 3792, b"ACGT")
        at = rng.randrange(3000)
        pairs.append((a, t[:at] + a + t[at + 100:]))
    assert all(len(b) == 3792 for _a, b in pairs)
    res = al.align_batch("edit", pairs, render=False)
    _check(res, pairs)
    with pytest.raises(A.AlignToolsError) as ei:
        al.align_batch("edit", [(pairs[0][0], pairs[0][1] + b"A")])
    assert ei.value.code == A.ERR_DOMAIN and "max_len2 = 3793" in str(ei.value), ei.value


@pytest.mark.gpu
def test_domain(al, one_chunk):
    rng = random.Random(5)
    pairs = [(_rand(rng, 40, b"ACGT"), _rand(rng, 44, b"ACGT")) for _ in range(5)]
    try:
        al.set_scoring(1, -2, -5, -1, -10)
        with pytest.raises(A.AlignToolsError) as ei:
            al.align_batch("edit", pairs)
        assert ei.value.code == A.ERR_DOMAIN and "u = -2" in str(ei.value), ei.value
    finally:
        al.set_scoring(*UNIT)
    with pytest.raises(A.AlignToolsError) as ei:
        al.align_batch("edit", pairs + [(b"ACGTNACGT", b"ACGTACGT")])
    assert ei.value.code == A.ERR_DOMAIN and "ACGT" in str(ei.value), ei.value
    with pytest.raises(A.AlignToolsError) as ei:
        al.align_batch("edit", pairs + [(_rand(rng, 1025, b"ACGT"), b"ACGT")])
    assert ei.value.code == A.ERR_DOMAIN and "max_len1 = 1025" in str(ei.value), ei.value
    for call in (al.align_batch_strings, al.align_batch_cigar):
        with pytest.raises(A.AlignToolsError) as ei:
            call("edit", pairs + [(b"ACGTNACGT", b"ACGTACGT")])
        assert ei.value.code == A.ERR_DOMAIN, ei.value
    _check(al.align_batch("edit", pairs, render=False), pairs, "after the refusals")
    # the setting off: everything as before
    al.set_edit_traceback(False)
    try:
        with pytest.raises(A.AlignToolsError) as ei:
            al.align_batch_strings("edit", pairs)
        assert ei.value.code == A.ERR_ARG and "edit has no alignment strings (alignment.h:291)" in str(ei.value)
        with pytest.raises(A.AlignToolsError) as ei:
            al.align_batch_cigar("edit", pairs)
        assert ei.value.code == A.ERR_ARG and "edit has no alignment, hence no CIGAR (alignment.h:291)" in str(ei.value)
        r = al.align_batch("edit", pairs)
        assert "ops" not in r and not r["nops"].any()
        assert [int(x) for x in r["score"]] == [_edit_ref(a, b)[0] for a, b in pairs]
    finally:
        al.set_edit_traceback(True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_entry(al, n):
    """Slots in shuffled order with guard bytes between and behind them: only nops[k] bytes of a slot change; a pair longer than
    max_len1 comes back refused with its slot untouched"""
    import torch
    rng = random.Random(60 + n)
    max1, max2 = 90, 120
    pairs = []
    for _ in range(n):
        a = _rand(rng, rng.randint(1, max1), b"ACGT")
        pairs.append((a, _related(rng, a, rng.randint(1, max2), b"ACGT")))
    long_k = 5 if n > 5 else -1
    if long_k >= 0:
        pairs[long_k] = (_rand(rng, max1 + 7, b"ACGT"), pairs[long_k][1])
    words, woff1, woff2, len1, len2, bits = A.pack_pairs(pairs)
    assert bits == 2
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("w", words.view(np.int32)), ("o1", woff1), ("o2", woff2), ("l1", len1), ("l2", len2))}
    slot = max1 + 7 + max2 + 9                          # a pair's ops and a guard of at least nine bytes
    perm = list(range(n))
    rng.shuffle(perm)
    ops_off = np.array([16 + perm[k] * slot for k in range(n)], dtype=np.int64)
    ops = torch.full((16 + n * slot + 64,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.full((5, n), -7, dtype=torch.int32, device=dev)
    d_off = torch.from_numpy(ops_off).to(dev)
    al.align_batch_device(A.MODE_EDIT, n, d["w"].data_ptr(), bits, d["o1"].data_ptr(), d["l1"].data_ptr(), d["o2"].data_ptr(),
                          d["l2"].data_ptr(), max1, max2, False, True, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                          out[3].data_ptr(), ops.data_ptr(), d_off.data_ptr(), out[4].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert al.last_config.startswith("myers-tb bits=2 words/lane=3 "), al.last_config
    o = out.cpu().numpy()
    got = ops.cpu().numpy()
    want = np.full(len(got), 0xEE, dtype=np.uint8)
    for k, (a, b) in enumerate(pairs):
        if k == long_k:
            assert (int(o[0][k]), int(o[4][k])) == (INT32_MIN, -1)
            continue
        dist, ref = _edit_ref(a, b)
        assert (int(o[0][k]), int(o[1][k]), int(o[2][k]), int(o[3][k]), int(o[4][k])) == (dist, len(a), len(b), A.ST_MID, len(ref)), k
        want[ops_off[k]:ops_off[k] + len(ref)] = np.frombuffer(ref, dtype=np.uint8)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_forms(al, one_chunk):
    """The strings form is the rendering of the ops, the CIGAR form their host CIGAR; the statistics rows add up"""
    rng = random.Random(7)
    pairs = [(b"", b"ACG"), (b"ACGT", b"ACGT")]
    while len(pairs) < 90:
        a = _rand(rng, rng.randint(1, 200), b"ACGT")
        pairs.append((a, _related(rng, a, rng.randint(1, 220), b"ACGT")))
    ref = al.align_batch("edit", pairs, render=False)
    _check(ref, pairs)
    st = al.align_batch_strings("edit", pairs)
    assert "myers-tb" in al.last_config and "[strings: " in al.last_config, al.last_config
    cg = al.align_batch_cigar("edit", pairs)
    assert "myers-tb" in al.last_config and "[cigar: " in al.last_config, al.last_config
    for k, (a, b) in enumerate(pairs):
        r1, r2 = al.render(ref["ops"][k], a, len(a), b, len(b))
        assert (st["r1"][k], st["r2"][k], int(st["nops"][k]), int(st["score"][k])) == (r1, r2, len(r1), int(ref["score"][k])), k
        assert r1.replace("-", "").encode() == a and r2.replace("-", "").encode() == b, k
        words, stats = A.cigar(ref["ops"][k], a, len(a), b, len(b))
        assert cg["cigar"][k].tolist() == words.tolist() and cg["stats"][k].tolist() == stats.tolist(), k
        si, sj, eq, ne, ins, dele = (int(x) for x in cg["stats"][k][:6])
        assert (si, sj) == (0, 0) and ne + ins + dele == int(cg["score"][k]) == int(ref["score"][k]), k
        assert eq + ne + ins == len(a) and eq + ne + dele == len(b), k


@pytest.mark.gpu
def test_chunked_host_path(al, monkeypatch):
    """2 x AT_HOST_CHUNK_MIN + 7 pairs: the helper handles of the chunks honour the setting"""
    monkeypatch.setenv("AT_HOST_CHUNK_MIN", "1024")
    rng = random.Random(8)
    pairs = []
    for _ in range(2 * 1024 + 7):
        a = _rand(rng, 36, b"ACGT")
        pairs.append((a, _related(rng, a, 36, b"ACGT")))
    res = al.align_batch("edit", pairs, render=False)
    assert "myers-tb" in al.last_config and " x2 chunks" in al.last_config, al.last_config
    _check(res, pairs)
    st = al.align_batch_strings("edit", pairs[:2 * 1024 + 1])
    assert " x2 chunks" in al.last_config, al.last_config
    for k in range(2 * 1024 + 1):
        assert (st["r1"][k], st["r2"][k]) == al.render(res["ops"][k], pairs[k][0], 36, pairs[k][1], 36), k
