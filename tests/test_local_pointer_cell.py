"""The pointer cells of the one-pass local kernels with scores x16 (at_sweep16.hip.h, PtrTags): tags L 12 / M 6 / U 3, the cell
m ^ ~(l | u) of the three words' low nibbles, and the walkers' decode of it (xor3_next; the table itself is proven at compile time).

Every pair of every batch against the oracle: score, end cell, start state, nops and every op.  The inputs make all 16 cell values
reachable and walked: unrelated reads (short walks, HOME cells), homopolymers and dinucleotide repeats (ties in every maximum), and
pairs X + Y against X + insert + Y and the reverse with inserts of 1, 3 and 10 bases (walks that open and extend gaps in L and in
U).  The shapes sit on the edges of every kernel class -- rows per lane of the 4-, 8-, 16- and 32-lane groups, several strips of
the 64-lane group -- in batches of 1, 17 and about a thousand pairs; then byte words, ragged frames, sliver items, and the two-pass
kernels, which keep the other tag set.
"""
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SCORINGS = [(2, -2, -5, -2), (1, -1, -1, -1)]     # the second: ties wherever two candidates can meet
J = -10
FLANK = 40
INSERTS = (1, 3, 10)

# l1 x l2 -> lanes per group (at_hip.hip, layout16_for): reads of up to 76 / 152 / 304 / 608 bases, then the 64-lane group in strips
SHAPES = [
    (1, 1), (36, 40), (76, 76),
    (77, 150), (104, 104), (105, 90), (128, 128), (129, 150), (150, 150), (152, 152),
    (153, 160), (304, 304),
    (305, 310),
    (700, 650),
]


def _lanes(l1):
    return 4 if l1 <= 76 else 8 if l1 <= 152 else 16 if l1 <= 304 else 32 if l1 <= 608 else 64


def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _pad(rng, core, n):
    """core somewhere inside n random bases (cut down if it is longer)"""
    core = core[:n]
    left = rng.randint(0, n - len(core))
    return _rnd(rng, left) + core + _rnd(rng, n - len(core) - left)


def _pair(rng, l1, l2, k):
    """pair k of a batch of l1 x l2; the kinds take turns"""
    kind = k % 8
    if kind == 0:
        return _rnd(rng, l1), _rnd(rng, l2)
    if kind == 1:                                   # homopolymers, one of them with a foreign base now and then
        s2 = list("A" * l2)
        for _ in range(k // 8 % 3):
            s2[rng.randrange(l2)] = "C"
        return "A" * l1, "".join(s2)
    if kind == 2:                                   # dinucleotide repeats, in and out of phase, one unit apart
        a, b = ("AC", "CA") if k // 8 % 2 else ("AC", "AC")
        s1, s2 = (a * l1)[:l1], list((b * l2)[:l2])
        if k // 16 % 2 and l2 > 4:
            del s2[l2 // 2:l2 // 2 + 1]             # (a one-base slip in the repeat: many gap placements of equal score)
            s2.append("A")
        return s1, "".join(s2)
    # X + Y against X + insert + Y (kinds 3, 4, 5: inserts of 1, 3, 10) and the reverse (6, 7, and 3 .. 5 in turn)
    ins = INSERTS[(k // 8 + kind) % 3]
    f = min(FLANK, (min(l1, l2) - ins) // 2)
    if f < 4:
        return _rnd(rng, l1), _rnd(rng, l2)
    x, y, gap = _rnd(rng, f), _rnd(rng, f), _rnd(rng, ins)
    short, long_ = x + y, x + gap + y
    if kind >= 6 or (k // 8) % 2:
        return _pad(rng, long_, l1), _pad(rng, short, l2)     # the insert in s1: a gap in s2
    return _pad(rng, short, l1), _pad(rng, long_, l2)


def _batch(rng, l1, l2, n):
    return [_pair(rng, l1, l2, k) for k in range(n)]


def _rep(uniq, n):
    return [uniq[k % len(uniq)] for k in range(n)]


_CACHE = {}


def _oracle(pairs, sc):
    """the restatement's result for every distinct pair, computed once per scoring and pair"""
    memo = _CACHE.setdefault(sc, {})
    todo = [p for p in dict.fromkeys(pairs) if p not in memo]
    if todo:
        O.align(O.LOCAL, "A", "AA")                 # (loads the library before the threads start)
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            res = list(ex.map(lambda p: O.align(O.LOCAL, p[0], p[1], *sc, J, False, []), todo))
        memo.update(zip(todo, res))
    return memo


def _run(al, pairs, sc, ctx=""):
    """align_batch (local, tracebacks) + every pair against the oracle.  Returns last_config."""
    al.set_scoring(*sc, J, False, [])
    res = al.align_batch("local", pairs, traceback=True, render=False)
    cfg = al.last_config
    ref = _oracle(pairs, sc)
    for k, p in enumerate(pairs):
        r = ref[p]
        where = (ctx, sc, k, len(p[0]), len(p[1]), cfg)
        assert r["rc"] == 0, where
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]), int(res["nops"][k]))
        assert got == (r["score"], r["end_i"], r["end_j"], r["state"], len(r["ops"])), where
        assert res["ops"][k] == r["ops"], where
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
    """monkeypatch with one chunk per host-entry call (a chunk on a helper handle would keep its own last_config); one-pass kernels"""
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    for name in ("AT_TP_SPLIT", "AT_GROUP", "AT_STORE", "AT_NO_PACKED", "AT_WS_CAP_MB", "AT_WALK_TEAMS", "AT_CK_PIECE_PAIRS", "AT_TAIL_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("AT_TWO_PASS", "0")
    return monkeypatch


def test_inputs_walk_gaps_in_both_states():
    """A condition on the inputs (oracle only): the insert pairs' walks hold runs of L ops and of U ops of every insert length, that is
    cells where a gap opened and cells where it extended, in both states; the unrelated pairs end at HOME after a short walk."""
    rng = random.Random(7)
    pairs = _batch(rng, 150, 150, 96)
    ref = _oracle(pairs, SCORINGS[0])
    runs = {1: set(), 2: set()}
    for p in pairs:
        for op in (1, 2):
            runs[op] |= {len(m) for m in re.findall(bytes([op]) + b"+", ref[p]["ops"])}
    assert set(INSERTS) <= runs[1] and set(INSERTS) <= runs[2], runs
    assert any(0 < len(ref[p]["ops"]) < 40 for p in pairs[0::8])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_local_one_pass_matches_oracle(al, env, shape):
    """batches of 1, 17 and 1 003 pairs (an odd count: the last work item is not full) of one shape, both scorings"""
    l1, l2 = shape
    rng = random.Random(l1 * 1000 + l2)
    uniq = _batch(rng, l1, l2, 32 if l1 > 304 else 96)
    for sc in SCORINGS:
        for n in (1, 17, 1003):
            cfg = _run(al, _rep(uniq, n) if n > 1 else uniq[3:4], sc, ctx=(shape, n))
            if n == 1003:
                g = _lanes(l1)
                assert "packed16 x16 " in cfg and "%dx%d-lane groups" % (64 // g, g) in cfg and "two-pass" not in cfg, cfg


def test_bytes_words(al, env):
    """an N in a read: the batch travels as byte words (compare instead of the score LUT)"""
    rng = random.Random(11)
    pairs = _batch(rng, 150, 150, 96)
    s1, s2 = pairs[5]
    pairs[5] = (s1[:70] + "N" + s1[71:], s2)
    s1, s2 = pairs[30]
    pairs[30] = (s1, s2[:20] + "NN" + s2[22:])
    for sc in SCORINGS:
        cfg = _run(al, _rep(pairs, 500), sc, ctx="bytes")
        assert "packed16 x16 bits=8 " in cfg and "8x8-lane groups" in cfg and "two-pass" not in cfg, cfg


def test_ragged_frames(al, env):
    """reads of 100 .. 150 bases through the host entry: ragged frames (fillers, columns and rows behind an alignment's own extents)"""
    rng = random.Random(13)
    pairs = [_pair(rng, rng.randint(100, 150), rng.randint(100, 150), k) for k in range(300)]
    for sc in SCORINGS:
        cfg = _run(al, pairs, sc, ctx="ragged")
        assert "packed16 x16 " in cfg and "ragged frames" in cfg, cfg


def test_sliver_as_32_lane_items(al, env):
    """The construction of tests/test_dense_sites.py::test_sliver_as_32_lane_items_with_the_jump_state in local mode at 150 x 150: a cap
    on the workspace shrinks the grid to g waves (the smallest number of MB that holds five pointer slots, from the slot size a probe
    reports), then three rounds of 8-lane items and one more item's worth, which goes to 32-lane items: both kinds of item write and
    walk the new cells."""
    rng = random.Random(17)
    uniq = _batch(rng, 150, 150, 96)
    sc = SCORINGS[0]
    probe = _run(al, uniq[:40], sc, ctx="probe")
    slot = int(re.search(r"slot=(\d+)B", probe).group(1))
    cap_mb = -(-5 * slot >> 20)
    g = (cap_mb << 20) // slot
    assert 5 <= g <= 16, probe
    env.setenv("AT_WS_CAP_MB", str(cap_mb))
    cfg = _run(al, _rep(uniq, 16 * (3 * g + 1) - 7), sc, ctx="sliver")
    assert "8x8-lane groups" in cfg and int(re.search(r"grid=(\d+)", cfg).group(1)) == g, cfg
    assert re.search(r"last 9 pairs as 32-lane items", cfg), cfg


def test_two_pass_kernels_keep_their_cells(al, env):
    """AT_TWO_PASS=2: the sweep without pointers, cells rebuilt by the replay and walked with the tags L 15 / M 10 / U 1 -- the rounds
    inside the sweep's kernel and the walk kernel"""
    rng = random.Random(19)
    pairs = _rep(_batch(rng, 150, 150, 96), 500)
    env.setenv("AT_TWO_PASS", "2")
    for split, text in (("0", "two-pass ck="), ("1", "two-pass (walk kernel)")):
        env.setenv("AT_TP_SPLIT", split)
        for sc in SCORINGS:
            cfg = _run(al, pairs, sc, ctx="two-pass " + split)
            assert "packed16 x16 " in cfg and "8x8-lane groups" in cfg and text in cfg, cfg
