"""The one-pass local kernels with the profile lookup and tracebacks (at_sweep16.hip.h, MAX3): the cell maximum X = max(L, M, U) as one
three-input float maximum on scores that carry a bias of 0x4000 in the L, U and X domain.  Every pair of every batch goes against the oracle
-- score, end cell, start state, nops and every op -- as in tests/test_local_step_diet.py.

Where it can go wrong: a half that leaves [0x0400, 0x7BFF] (NaN or infinity patterns: the highest scores of identical reads at the last
admitted m * min(l1, l2), the lowest L and U under a large |o|), a border that misses its bias (every group width, the boundary row of the
multi-strip 64-lane kernel, the constant border of the others, lanes with masked rows), ties that only the tags decide (reads with no common
base: every M clamps and X sits on the bias itself; repeats), and the route: a batch outside the domain must run the LUT kernels.
"""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SC = (2, -2, -5, -2)
BIASED = "[profile words, biased max3]"
LUT = "[score LUT]"
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _fit(s, l, rng):
    """s cut or filled up with random bases to l bases"""
    if s.size >= l:
        return s[:l]
    return np.concatenate([s, _ACGT[rng.integers(0, 4, size=l - s.size)]])


def _related(s1, l2, rng):
    keep = s1[rng.random(s1.size) >= 0.03].copy()
    sub = rng.random(keep.size) < 0.05
    keep[sub] = _ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    where = np.flatnonzero(rng.random(keep.size) < 0.03)
    return _fit(np.insert(keep, where, _ACGT[rng.integers(0, 4, size=where.size)]), l2, rng)


def _content(l1, l2, n, seed):
    """n pairs of l1 x l2, a fifth of each kind: related reads (substitutions and short gaps); identical reads (the longest walks, the
    highest scores); reads with no common base (every M clamps: X is the bias plus a tag everywhere); one long insertion and one long
    deletion (L and U chains at their lowest); repeats of period 1 .. 3 with a few substitutions (ties)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 5
        s1 = _ACGT[rng.integers(0, 4, size=l1)]
        if kind == 0:
            s2 = _related(s1, l2, rng)
        elif kind == 1:
            s2 = _fit(s1, l2, rng)
        elif kind == 2:
            s1 = _ACGT[rng.integers(0, 2, size=l1)]
            s2 = _ACGT[rng.integers(2, 4, size=l2)]
        elif kind == 3:
            g = max(1, min(l1, l2) // 7)
            a, b = l1 // 3, 2 * l1 // 3
            s2 = _fit(np.concatenate([s1[:a], _ACGT[rng.integers(0, 4, size=g)], s1[a:b], s1[min(l1, b + g):]]), l2, rng)
        else:
            p = int(rng.integers(1, 4))
            unit = _ACGT[rng.integers(0, 4, size=p)]
            s1 = np.tile(unit, l1 // p + 1)[:l1].copy()
            s2 = np.tile(unit, l2 // p + 1)[:l2].copy()
            for s in (s1, s2):
                hit = rng.random(s.size) < 0.04
                s[hit] = _ACGT[rng.integers(0, 4, size=int(hit.sum()))]
        out.append((s1.tobytes(), s2.tobytes()))
    return out


_CACHE = {}


def _oracle(pairs, sc):
    """the oracle's result for every distinct pair, once per scoring and pair"""
    memo = _CACHE.setdefault(sc, {})
    todo = [p for p in dict.fromkeys(pairs) if p not in memo]
    if todo:
        O.align(O.LOCAL, b"A", b"AA")               # (loads the library before the threads start)
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            res = list(ex.map(lambda p: O.align(O.LOCAL, p[0], p[1], *sc), todo))
        memo.update(zip(todo, res))
    return [memo[p] for p in pairs]


def _compare(res, ops_of, pairs, sc, tb, where):
    ref = _oracle(pairs, sc)
    assert all(r["rc"] == 0 for r in ref), where
    for key in ("score", "end_i", "end_j"):
        want = np.array([r[key] for r in ref])
        bad = np.flatnonzero(np.asarray(res[key]) != want)
        assert bad.size == 0, (key, int(bad[0]), int(np.asarray(res[key])[bad[0]]), int(want[bad[0]]), where)
    if tb:
        for key, want in (("state", [r["state"] for r in ref]), ("nops", [len(r["ops"]) for r in ref])):
            bad = np.flatnonzero(np.asarray(res[key]) != np.array(want))
            assert bad.size == 0, (key, int(bad[0]), where)
        for k, r in enumerate(ref):
            assert ops_of(k) == r["ops"], (k, where)


def _check(al, pairs, sc, tb, ctx):
    """align_batch (local) against the oracle, every pair.  Returns last_config."""
    al.set_scoring(*sc)
    res = al.align_batch("local", pairs, traceback=tb, render=False)
    cfg = al.last_config
    _compare(res, lambda k: res["ops"][k], pairs, sc, tb, (ctx, sc, tb, cfg))
    return cfg


def _check_device(al, pairs, sc, tb, ctx):
    """the same through at_align_batch_device with 2-bit words (the host entry sends scores of 8 and more as byte words, which have no
    profile form): pairs of one shape.  Returns last_config."""
    import torch
    import aligntools.c_amd as A
    from aligntools.c_amd import synth as S
    n, l1, l2 = len(pairs), len(pairs[0][0]), len(pairs[0][1])
    dev = torch.device("cuda", 0)
    lut = np.zeros(256, dtype=np.uint8)
    lut[_ACGT] = np.arange(4)
    codes = torch.from_numpy(lut[np.frombuffer(b"".join(a + b for a, b in pairs), dtype=np.uint8)].reshape(n, l1 + l2)).to(dev)
    w1, w2 = (l1 + 15) // 16 + 1, (l2 + 15) // 16 + 1
    d_words = torch.empty((n, w1 + w2), dtype=torch.int32, device=dev)
    d_words[:, :w1] = S.pack2_torch(codes[:, :l1])
    d_words[:, w1:] = S.pack2_torch(codes[:, l1:])
    base = torch.arange(n, dtype=torch.int64, device=dev) * (w1 + w2)
    d_woff1, d_woff2 = base, base + w1
    d_len1 = torch.full((n,), l1, dtype=torch.int32, device=dev)
    d_len2 = torch.full((n,), l2, dtype=torch.int32, device=dev)
    d_ops_off = torch.arange(n, dtype=torch.int64, device=dev) * (l1 + l2)
    d_ops = torch.zeros(n * (l1 + l2) + 64, dtype=torch.uint8, device=dev)
    out = torch.zeros((5, n), dtype=torch.int32, device=dev)
    al.set_scoring(*sc)
    al.align_batch_device(A.MODE_LOCAL, n, d_words.data_ptr(), 2, d_woff1.data_ptr(), d_len1.data_ptr(), d_woff2.data_ptr(),
                          d_len2.data_ptr(), l1, l2, True, tb, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                          out[3].data_ptr(), d_ops.data_ptr(), d_ops_off.data_ptr(), out[4].data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cfg = al.last_config
    h = out.cpu().numpy()
    ops2d = d_ops[:n * (l1 + l2)].view(n, l1 + l2).cpu().numpy()
    res = {"score": h[0], "end_i": h[1], "end_j": h[2], "state": h[3], "nops": h[4]}
    _compare(res, lambda k: ops2d[k, :h[4, k]].tobytes(), pairs, sc, tb, (ctx, sc, tb, cfg))
    return cfg


@pytest.fixture(scope="module")
def al():
    import aligntools.c_amd as A
    before = os.environ.get("AT_PACKED_MIN_ROUNDS")
    os.environ["AT_PACKED_MIN_ROUNDS"] = "0"   # small test batches must still reach the 64-lane packed kernels
    a = A.Aligner()
    yield a
    a.close()
    if before is None:
        os.environ.pop("AT_PACKED_MIN_ROUNDS", None)
    else:
        os.environ["AT_PACKED_MIN_ROUNDS"] = before


@pytest.fixture
def env(monkeypatch):
    """one chunk per host-entry call (a chunk on a helper handle would keep its own last_config); one-pass kernels"""
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    for name in ("AT_TP_SPLIT", "AT_GROUP", "AT_STORE", "AT_NO_PACKED", "AT_WS_CAP_MB", "AT_WALK_TEAMS", "AT_CK_PIECE_PAIRS", "AT_TAIL_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("AT_TWO_PASS", "0")
    return monkeypatch


@pytest.mark.parametrize("case", [(76, 150, None, 4), (150, 150, None, 8), (152, 149, None, 8), (150, 150, "16", 16), (250, 150, "32", 32)],
                         ids=lambda c: "%dx%d-g%d" % (c[0], c[1], c[3]))
def test_every_group_width(al, env, case):
    """every kind of content on every group width below 64 lanes (the constant border); with tracebacks the biased kernel, without them
    the scores-only profile kernel, which is what it was"""
    l1, l2, group, g = case
    if group:
        env.setenv("AT_GROUP", group)
    pairs = _content(l1, l2, 1000, 0x3A30 + 1000 * l1 + l2 + g)
    ref = _oracle(pairs, SC)
    assert max(r["score"] for r in ref) == 2 * min(l1, l2) and min(r["score"] for r in ref) == 0      # identical reads; no common base
    assert max(len(r["ops"]) for r in ref) >= min(l1, l2)
    for tb, form in ((True, BIASED), (False, "[profile words]")):
        cfg = _check(al, pairs, SC, tb, case)
        assert "packed16 x16 bits=2 %dx%d-lane groups" % (64 // g, g) in cfg and form in cfg and "two-pass" not in cfg, cfg


def test_multi_strip_64_lane_kernel(al, env):
    """700 x 700 under m = 1 on one group of 64 lanes: two strips, the boundary row between them written back and read again biased"""
    env.setenv("AT_GROUP", "64")
    sc = (1, -1, -2, -1)
    pairs = _content(700, 700, 200, 0x700)
    assert max(r["score"] for r in _oracle(pairs, sc)) == 700
    cfg = _check(al, pairs, sc, True, "64 lanes")
    assert "packed16 x16 bits=2 1x64-lane groups" in cfg and BIASED in cfg and "two-pass" not in cfg, cfg


@pytest.mark.parametrize("l1", [1, 19, 20])
def test_first_lanes_and_masked_rows(al, env, l1):
    """one row, one lane's rows, one row more: lanes that own no row, a last lane with masked rows"""
    env.setenv("AT_GROUP", "8")
    for l2 in (7, 150):
        cfg = _check(al, _content(l1, l2, 500, 0x1A0 + 10 * l1 + l2), SC, True, (l1, l2))
        assert "8x8-lane groups" in cfg and BIASED in cfg, cfg


def test_sliver_of_32_lane_items(al, env):
    """a whole round for every resident wave and an eighth more: the last round goes to items of two 32-lane groups in the same launch"""
    uniq = _content(150, 150, 1500, 0x511)
    al.set_scoring(*SC)
    al.align_batch("local", uniq * 40, traceback=True, render=False)     # one full-size call tells the grid of this kernel on this chip
    grid = int(re.search(r" grid=(\d+)", al.last_config).group(1))
    n = 16 * (grid + grid // 8)
    pairs = (uniq * (n // len(uniq) + 1))[:n]
    cfg = _check(al, pairs, SC, True, "sliver")
    assert "8x8-lane groups" in cfg and "pairs as 32-lane items" in cfg and BIASED in cfg, cfg


def test_ragged_batch(al, env):
    """the pairs of a 150 x 150 frame at lengths of their own: the ragged kernels, masked rows and columns, the frame decides the route"""
    pairs = _content(150, 150, 900, 0x4A66)
    rng = np.random.default_rng(0x4A67)
    a = rng.integers(1, 151, size=len(pairs))
    b = rng.integers(1, 151, size=len(pairs))
    a[:5], b[:5] = 150, 150
    ragged = [(s1[:int(x)], s2[:int(y)]) for (s1, s2), x, y in zip(pairs, a, b)]
    cfg = _check(al, ragged, SC, True, "ragged")
    assert "packed16 x16 bits=2 " in cfg and "ragged frames" in cfg and BIASED in cfg, cfg


@pytest.mark.parametrize("case", [((2, -2, -5, -2), 472, False), ((1, -1, -2, -1), 944, False), ((15, 0, -5, -2), 62, True), ((8, -7, -9, -2), 118, True)],
                         ids=lambda c: "m%d-l%d" % (c[0][0], c[1]))
def test_last_admitted_score_and_one_past(al, env, case):
    """m * min(l1, l2) = 944 (or the last multiple of m below it) is the last value admitted: identical reads reach it.  One base more and
    the batch keeps the LUT kernels.  Both match the oracle.  (Scores of 8 and more: 2-bit words through the device entry.)"""
    sc, l, device = case
    n = 100 if l > 500 else 300
    for ll, form in ((l, BIASED), (l + 1, LUT)):
        for l2 in (ll, ll + 9):
            pairs = _content(ll, l2, n, 0xED6E + 10 * ll + l2 + sc[0])
            assert max(r["score"] for r in _oracle(pairs, sc)) == sc[0] * ll
            cfg = (_check_device if device else _check)(al, pairs, sc, True, (case, ll, l2))
            assert "packed16 x16 bits=2 " in cfg and form in cfg and "two-pass" not in cfg, cfg


@pytest.mark.parametrize("case", [((2, -2, -60, -2), 150, 150, False, BIASED), ((2, -2, -5, 0), 150, 150, False, BIASED), ((0, 0, -1, -1), 150, 150, False, BIASED),
                                  ((8, -7, -9, -2), 100, 150, True, BIASED), ((2, -2, -955, -2), 20, 24, False, BIASED), ((2, -2, -956, -2), 20, 24, False, LUT),
                                  ((8, -8, -9, -2), 100, 150, True, LUT)],
                         ids=lambda c: "%d_%d_%d_%d-%dx%d" % (c[0] + (c[1], c[2])))
def test_scoring_at_the_edges(al, env, case):
    """a large |o| (L and U far below the bias; |o| + |u| + |e| = 959 is the last sum admitted), e = 0, m = u = 0 (every cell ties),
    8 / -7 (D = 240: the last profile byte) and 8 / -8 (D = 256: no profile words), the last two with 2-bit words through the device entry"""
    sc, l1, l2, device, form = case
    pairs = _content(l1, l2, 1000, 0x5C0 + l1 + l2 - sc[2])
    cfg = (_check_device if device else _check)(al, pairs, sc, True, case)
    assert "packed16 x16 bits=2 " in cfg and form in cfg and "two-pass" not in cfg, cfg
