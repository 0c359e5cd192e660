"""The one-pass local kernels of the groups below 64 lanes (at_sweep16.hip.h, DIET): the row above the strip as a constant instead of a
boundary row in LDS, the step number of the arg-max fold as a scalar operand.  Every pair of every batch goes against the oracle -- score,
end cell, start state, nops and every op -- as in tests/test_gpu_parity.py.  (The shapes also cover how a pointer word of four steps is put
together: a form of it with one instruction less was tried beside these two and dropped, profiles/LOG.md I.)

Where such edits can go wrong: a last pointer word of 1, 2 or 3 valid steps and lanes that sit out steps inside a word (l2 = 1, 2, 3, 4, 5,
7, 9); the first and last lane of a group and its masked rows (l1 = 1, 19, 20, 150, 151, 152 on the 8-lane groups); every group width; walks
that cross many words in all three states (s2 is a copy of s1 with substitutions, insertions and deletions); the profile form (2 / -2), the
LUT form (8 / -8 with 2-bit words, through the device entry) and byte words (8 / -8 through the host entry); a ragged batch; a batch whose last
round goes to the 32-lane items of the sliver; and one batch on the 64-lane kernel, whose strips still read their boundary row from LDS.
"""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SC_PROF = (2, -2, -5, -2)     # the profile words (and 2-bit sequence words through the host entry)
SC_WIDE = (8, -8, -9, -2)     # D = 256: the score LUT on 2-bit words (device entry); byte words through the host entry
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _related(l1, l2, n, seed):
    """n pairs of l1 x l2 as bytes: s2 is s1 with 5 % substitutions, 3 % insertions and 3 % deletions, cut or filled up to l2 bases"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s1 = _ACGT[rng.integers(0, 4, size=l1)]
        u = rng.random(l1)
        keep = s1[u >= 0.03].copy()
        sub = rng.random(keep.size) < 0.05
        keep[sub] = _ACGT[rng.integers(0, 4, size=int(sub.sum()))]
        where = np.flatnonzero(rng.random(keep.size) < 0.03)
        s2 = np.insert(keep, where, _ACGT[rng.integers(0, 4, size=where.size)])
        if s2.size > l2:
            off = int(rng.integers(0, s2.size - l2 + 1))
            s2 = s2[off:off + l2]
        else:
            s2 = np.concatenate([s2, _ACGT[rng.integers(0, 4, size=l2 - s2.size)]])
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


def _check(al, pairs, sc, tb, ctx):
    """align_batch (local) against the oracle, every pair.  Returns last_config."""
    al.set_scoring(*sc)
    res = al.align_batch("local", pairs, traceback=tb, render=False)
    cfg = al.last_config
    ref = _oracle(pairs, sc)
    where = (ctx, sc, tb, cfg)
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
            assert res["ops"][k] == r["ops"], (k, where)
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


@pytest.mark.parametrize("l1", [1, 19, 20, 150, 151, 152])
def test_short_targets_on_8_lane_groups(al, env, l1):
    """l2 of 1 .. 9 columns: one to three pointer words per row, the last one with 1, 2 or 3 valid steps; with the lanes' ramp every
    lane but the first sits out steps inside its first and last words"""
    env.setenv("AT_GROUP", "8")
    for l2 in (1, 2, 3, 4, 5, 7, 9):
        pairs = _related(l1, l2, 500, 0xD1E7 + 1000 * l1 + l2)
        for tb in (True, False):
            cfg = _check(al, pairs, SC_PROF, tb, (l1, l2))
            assert "packed16 x16 bits=2 8x8-lane groups" in cfg and "two-pass" not in cfg, cfg


@pytest.mark.parametrize("case", [(150, 150, None, 8), (152, 149, None, 8), (151, 163, None, 8), (76, 150, None, 4), (150, 150, "16", 16),
                                  (250, 150, "32", 32)], ids=lambda c: "%dx%d-g%d" % (c[0], c[1], c[3]))
def test_long_walks_every_group_width(al, env, case):
    """related pairs: walks of a hundred ops and more through all three states, on 2-bit words (profile form) and on byte words"""
    l1, l2, group, g = case
    if group:
        env.setenv("AT_GROUP", group)
    pairs = _related(l1, l2, 1500, 0x10A6 + 1000 * l1 + l2 + g)
    assert np.mean([len(r["ops"]) for r in _oracle(pairs[:200], SC_PROF)]) > 0.4 * min(l1, l2)
    for sc, words in ((SC_PROF, "bits=2 "), (SC_WIDE, "bits=8 ")):
        for tb in (True, False):
            cfg = _check(al, pairs, sc, tb, case)
            assert "packed16 x16 " + words in cfg and "two-pass" not in cfg, cfg
            assert "%dx%d-lane groups" % (64 // g, g) in cfg or (g == 32 and sc is SC_WIDE), cfg   # (byte words: no 32-lane class of their own)


def test_ragged_batch(al, env):
    """the pairs of a 150 x 150 frame at lengths of their own: the ragged kernels (16-lane groups), masked rows and columns"""
    pairs = _related(150, 150, 900, 0x4A66)
    rng = np.random.default_rng(0x4A67)
    a = rng.integers(1, 151, size=len(pairs))
    b = rng.integers(1, 151, size=len(pairs))
    a[0], b[0] = 150, 150
    ragged = [(s1[:int(x)], s2[:int(y)]) for (s1, s2), x, y in zip(pairs, a, b)]
    for sc, words in ((SC_PROF, "bits=2 "), (SC_WIDE, "bits=8 ")):
        for tb in (True, False):
            cfg = _check(al, ragged, sc, tb, "ragged")
            assert "packed16 x16 " + words in cfg and "ragged frames" in cfg, cfg


def test_sliver_of_32_lane_items(al, env):
    """a whole round for every resident wave and an eighth more: the last round, less than a quarter full, goes to items of two 32-lane
    groups in the same launch (5 rows per lane, two pointer words per block of steps)"""
    uniq = _related(150, 150, 1500, 0x511)
    for tb in (True, False):
        al.set_scoring(*SC_PROF)
        al.align_batch("local", uniq * 40, traceback=tb, render=False)     # one full-size call tells the grid of this kernel on this chip
        grid = int(re.search(r" grid=(\d+)", al.last_config).group(1))
        n = 16 * (grid + grid // 8)
        pairs = (uniq * (n // len(uniq) + 1))[:n]
        cfg = _check(al, pairs, SC_PROF, tb, "sliver")
        assert "8x8-lane groups" in cfg and "pairs as 32-lane items" in cfg, cfg


@pytest.mark.parametrize("shape", [(150, 150), (150, 7), (250, 150)], ids=lambda s: "%dx%d" % s)
def test_device_entry_score_lut(al, env, shape):
    """at_align_batch_device with 2-bit words under 8 / -8 (D = 256: the score LUT) and under 2 / -2 (the profile words)"""
    import torch
    import aligntools.c_amd as A
    from aligntools.c_amd import synth as S
    l1, l2 = shape
    n = 1000
    pairs = _related(l1, l2, n, 0xDE71 + l1 + l2)
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
    for sc in (SC_WIDE, SC_PROF):
        ref = _oracle(pairs, sc)
        al.set_scoring(*sc)
        for tb in (True, False):
            d_ops = torch.zeros(n * (l1 + l2) + 64, dtype=torch.uint8, device=dev)
            res = torch.zeros((5, n), dtype=torch.int32, device=dev)
            al.align_batch_device(A.MODE_LOCAL, n, d_words.data_ptr(), 2, d_woff1.data_ptr(), d_len1.data_ptr(), d_woff2.data_ptr(),
                                  d_len2.data_ptr(), l1, l2, True, tb, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(),
                                  res[3].data_ptr(), d_ops.data_ptr(), d_ops_off.data_ptr(), res[4].data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            cfg = al.last_config
            assert "packed16 x16 bits=2 " in cfg and "two-pass" not in cfg, cfg
            h = res.cpu().numpy()
            ops2d = d_ops[:n * (l1 + l2)].view(n, l1 + l2).cpu().numpy()
            for k, r in enumerate(ref):
                assert (int(h[0, k]), int(h[1, k]), int(h[2, k])) == (r["score"], r["end_i"], r["end_j"]), (shape, sc, tb, k, cfg)
                if tb:
                    assert (int(h[3, k]), ops2d[k, :h[4, k]].tobytes()) == (r["state"], r["ops"]), (shape, sc, tb, k, cfg)


def test_multi_strip_64_lane_kernel_keeps_its_boundary_row(al, env):
    """reads of 700 bases on one group of 64 lanes: several strips per alignment, each reading the row above it from LDS"""
    env.setenv("AT_GROUP", "64")
    pairs = _related(700, 150, 96, 0x700)
    for tb in (True, False):
        cfg = _check(al, pairs, SC_PROF, tb, "64 lanes")
        assert "packed16 x16 bits=2 1x64-lane groups" in cfg and "two-pass" not in cfg, cfg
