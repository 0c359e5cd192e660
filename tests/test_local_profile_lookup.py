"""The diagonal candidate of the packed local kernels by the step's profile words (at_sweep16.hip.h, PROF: v_perm_b32, v_pk_add_u16,
v_pk_sub_u16 with clamp) for the scorings with m >= 0 >= u and (m - u) * 16 <= 255, and by the score LUT for every other scoring: the host
chooses between the two kernels of a class (at_hip.hip), the results are the same.  The identity itself is proven at compile time
(prof_proof); here every pair of every batch goes against the oracle -- score, end cell, start state, nops and every op -- as in
tests/test_gpu_parity.py.

Shapes: a single cell, a single row, one row per lane of the 4-lane groups' 19-row class and one more, the last lane's masked rows (37, 150
of 152), the full frame of the 8-lane groups (152).  About 2 000 pairs each, half unrelated, half mutate_pairs; the same pairs cut to
lengths of their own as a ragged batch; with and without tracebacks; every lane-group width AT_GROUP reaches for the shape.  Scorings:
the default, an uneven one, u = 0 (ties everywhere), m = 0, D = 240 with m = 8 (the last one inside the condition) and D = 256 (the first
one outside).  The host entry sends a scoring with |16 m| or |16 u| above 127 as byte words (scores_fit_byte), whose kernels compare
instead of looking up, so there those two run on the byte kernels and 7 / -8 is D = 240 on the 2-bit ones; a caller of the device entry
who hands over 2-bit words under such a scoring gets the 2-bit kernels (test_device_entry_two_bit_words_large_scores): D = 240 with the
profile words, D = 256 with the score LUT.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SCORINGS = [(2, -2, -5, -2), (1, -2, -5, -1), (1, 0, -1, -1), (0, -3, -4, -1), (8, -7, -9, -2), (8, -8, -9, -2),
            (7, -8, -9, -2)]


def _words(sc):
    """the sequence words the host entry packs a batch in under this scoring"""
    return "bits=2 " if abs(16 * sc[0]) <= 127 and abs(16 * sc[1]) <= 127 else "bits=8 "


SHAPES = [(1, 1), (1, 40), (19, 19), (20, 21), (37, 150), (150, 150), (152, 9)]
N = 2000
NRAG = 600


def _pairs(l1, l2, n, seed):
    """n pairs of l1 x l2 as bytes: the even ones unrelated, the odd ones s2 a substituted copy of s1 (mutate_pairs)"""
    from aligntools.c_amd.synth import synth_pairs_blob, mutate_pairs
    blob = synth_pairs_blob(seed, n, l1, l2)
    rel = mutate_pairs(blob, l1, l2, seed & 0xffff, sub=0.06)
    out = []
    for k in range(n):
        row = rel[k] if k % 2 else blob[k]
        out.append((row[:l1].tobytes(), row[l1:].tobytes()))
    return out


def _cut(pairs, l1, l2):
    """the pairs at lengths of their own inside the frame l1 x l2 (the first one keeps the frame's)"""
    rng = np.random.default_rng(l1 * 1000 + l2)
    a = rng.integers(1, l1 + 1, size=len(pairs))
    b = rng.integers(1, l2 + 1, size=len(pairs))
    a[0], b[0] = l1, l2
    return [(s1[:int(x)], s2[:int(y)]) for (s1, s2), x, y in zip(pairs, a, b)]


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


def _widths(l1):
    """(AT_GROUP, lanes per group) a uniform batch of l1-base reads can be sent to (at_hip.hip, layout16_for)"""
    return ([(None, 4), ("8", 8)] if l1 <= 76 else [(None, 8)]) + [("16", 16), ("64", 64)]


@pytest.mark.parametrize("sc", SCORINGS, ids=lambda s: "m%du%do%de%d" % s)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_local_batches_match_oracle(al, env, shape, sc):
    l1, l2 = shape
    pairs = _pairs(l1, l2, N, 0x10C0 + l1 * 1000 + l2)
    for group, g in _widths(l1):
        if group is None:
            env.delenv("AT_GROUP", raising=False)
        else:
            env.setenv("AT_GROUP", group)
        for tb in (True, False):
            cfg = _check(al, pairs, sc, tb, (shape, "uniform", g))
            assert "packed16 x16 " + _words(sc) in cfg and "%dx%d-lane groups" % (64 // g, g) in cfg and "two-pass" not in cfg, cfg
    env.delenv("AT_GROUP", raising=False)
    if l1 * l2 > 1:
        ragged = _cut(pairs[:NRAG], l1, l2)
        for tb in (True, False):
            cfg = _check(al, ragged, sc, tb, (shape, "ragged"))
            assert "packed16 x16 " + _words(sc) in cfg and "ragged frames" in cfg, cfg


@pytest.mark.parametrize("kind", ["identical", "mismatch"])
def test_all_identical_and_all_mismatch_batches(al, env, kind):
    """every cell of every matrix a match (the score climbs to m * l1: the largest sums the unsigned add sees), and every cell a
    mismatch (every diagonal candidate clamps to 0: HOME everywhere, score 0)"""
    for l1, l2 in ((150, 150), (37, 150)):
        if kind == "identical":
            base = _pairs(max(l1, l2), 1, 16, 0x1D)
            uniq = [(s[:l1], s[:l2]) for s, _ in base]
        else:
            uniq = [(bytes([a]) * l1, bytes([b]) * l2) for a in b"ACGT" for b in b"ACGT" if a != b]
        pairs = [uniq[k % len(uniq)] for k in range(203)]
        for sc in SCORINGS:
            for tb in (True, False):
                cfg = _check(al, pairs, sc, tb, (kind, l1, l2))
                assert "packed16 x16 " + _words(sc) in cfg and ("8x8-lane groups" if l1 > 76 else "16x4-lane groups") in cfg, cfg
            want = sc[0] * min(l1, l2) if kind == "identical" else 0
            assert _oracle(pairs[:1], sc)[0]["score"] == want


def test_32_lane_groups(al, env):
    """reads of 250 bases under AT_GROUP=32: two groups of 32 lanes x 8 rows (the sliver items' width as a batch of its own)"""
    pairs = _pairs(250, 60, 300, 0x3232)
    env.setenv("AT_GROUP", "32")
    for sc in SCORINGS:
        for tb in (True, False):
            cfg = _check(al, pairs, sc, tb, "32 lanes")
            if sc[0] <= 2:
                assert "packed16 x16 bits=2 " in cfg and "2x32-lane groups" in cfg, cfg


def test_two_pass_kernels(al, env):
    """AT_TWO_PASS=2: the forward sweep of the two-pass kernels and the replay inside them take the same candidate; the walk kernel
    (AT_TP_SPLIT=1) replays with the LUT"""
    pairs = _pairs(150, 150, 500, 0x2BA5)
    env.setenv("AT_TWO_PASS", "2")
    for split, text in (("0", "two-pass ck="), ("1", "two-pass (walk kernel)")):
        env.setenv("AT_TP_SPLIT", split)
        for sc in SCORINGS[2:]:
            cfg = _check(al, pairs, sc, True, "two-pass " + split)
            assert "packed16 x16 " in cfg and "8x8-lane groups" in cfg and text in cfg, cfg


@pytest.mark.parametrize("shape", [(150, 150), (37, 150), (250, 60)], ids=lambda s: "%dx%d" % s)
def test_device_entry_two_bit_words_large_scores(al, env, shape):
    """at_align_batch_device with 2-bit words, uniform shape, under 8 / -7 (D = 240: the profile words), 8 / -8 (D = 256: the score LUT,
    whose 16-bit entries hold 128 and -128) and 7 / -8: the 8-lane groups, and the 16-lane groups for 250-base reads; with and without
    tracebacks"""
    import torch
    import aligntools.c_amd as A
    from aligntools.c_amd import synth as S
    l1, l2 = shape
    n = 1000
    pairs = _pairs(l1, l2, n, 0xDE7 + l1)
    dev = torch.device("cuda", 0)
    lut = np.zeros(256, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
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
    for sc in SCORINGS[4:]:
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
