"""fit -s under DENSE site lists: every column listed except a few allowed ones.

The jump state may open at column j exactly when j - 1 is NOT in the site list (the reference's inverted test).  The
host turns the list into a bit mask (ensure_sitemask, bit j + 64) that every kernel family reads through window arithmetic of its
own.  With the handful of sites the other tests list, the jump may open almost anywhere, and a mask read one column off, a wrong
word, the other half's mask, a stale mask or no mask at all changes next to no result (3 pairs of 200 at 150 x 500 with sites
100|200|300|400 differ from the empty list).  Here the allowed columns are few, sit on both sides of the mask's word edges and at
both ends of s2, and three pairs of four are spliced reads whose first exon ends at or next to an allowed column: the exact column
decides the result.

  * the CPU half (no mark): the batches are sensitive -- at least half of the pairs change their result under the oracle when the
    list is shifted by +1, by -1, or emptied (a condition on the inputs, not on the code under test); metamorphic checks on the
    oracle; the oracle against the compiled reference (oracle/_ref, when present) and against tests/golden/dense_sites.jsonl
    (tests/test_oracle.py);
  * the GPU half (-m gpu): every kernel family, asserted from at_last_config, with every pair of every batch against the oracle:
    score, end_i, end_j, state, and ops when tracebacks are on.
"""
import os
import random
import re
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SCORINGS = [(2, -2, -5, -1, -10), (1, -1, -1, -1, 0), (2, -2, -5, -2, -3)]
CHEAP = SCORINGS[1:]          # where l2 < 1.5 l1 a jump of -10 hardly ever pays (10 pairs of 60 at 300 x 320): the two cheap jumps only
STORE_NAMES = {0: "store=lds ", 1: "store=lds+hbm-pointers ", 2: "store=hbm "}


# ---------------------------------------------------------------- generator

def allowed_columns(l2):
    """The values a dense list leaves out: c with (c + 65) % 32 in {31, 0, 1} -- the last bit of a mask word and the first two of the
    next, bit c + 65 being the one ensure_sitemask clears for a listed c -- at every second word edge, plus {0, l2 - 2, l2 - 1}."""
    a = {c for c in range(l2) if (c + 65) % 32 in (31, 0, 1) and ((c + 66) // 32) % 2 == 0}
    return a | {0, l2 - 2, l2 - 1}


def site_list(rng, l2, allowed):
    """Every integer of -2 .. l2 + 2 that is not allowed, shuffled, with a few duplicates: unsorted input, values outside the useful range"""
    sites = [c for c in range(-2, l2 + 3) if c not in allowed]
    sites += [rng.choice(sites) for _ in range(5)]
    rng.shuffle(sites)
    return sites


MIN_EXON = 12
SLIDE = 3


def _pair(rng, l1, l2, allowed, k, alpha="ACGT", unrelated_fourth=True):
    """pair k of a batch: a fresh contig of l2 bases; k % 4 == 3: an unrelated read; else a spliced read contig[b - x : b] +
    contig[c : c + l1 - x] whose first exon ends at b = an allowed column + delta (the jump opens from M(., b) iff b is not listed).
    Intron lengths c - b cycle through short (6 ..), more than 64 and more than 256 columns where l2 leaves room.
    The junction is ambiguous, as real ones are: the intron begins with the second exon's first SLIDE bases and ends with the first
    exon's last SLIDE bases, so the splice may slide by up to SLIDE columns either way at the same score.  The reference's first-wins
    ties then pick one of the columns the list allows in b - SLIDE .. b + SLIDE: which columns those are decides end cell and ops."""
    contig = [rng.choice(alpha) for _ in range(l2)]
    if (unrelated_fourth and k % 4 == 3) or l1 < 2 * MIN_EXON or l2 < l1 + 6:
        return "".join(rng.choice(alpha) for _ in range(l1)), "".join(contig)
    # an intron of 6 columns at least behind b, and both exons MIN_EXON bases at least
    cand = sorted(a for a in allowed if MIN_EXON + 2 <= a <= l2 - MIN_EXON - 8)
    for _ in range(64):
        b = (rng.choice(cand) if cand else rng.randint(MIN_EXON, l2 - MIN_EXON - 6)) + rng.choice([-2, -1, 0, 0, 1, 2])
        lo = max(MIN_EXON, l1 - (l2 - b - 6))
        hi = min(b, l1 - MIN_EXON)
        if lo <= hi:
            break
    else:
        return "".join(rng.choice(alpha) for _ in range(l1)), "".join(contig)
    want = (6, 65, 257)[(k // 4) % 3]                       # the intron class this pair aims at
    room = l2 - b - MIN_EXON                                # the longest intron that leaves a second exon
    x_lo = lo if room < want else max(lo, min(hi, l1 - (l2 - b - want)))
    x = rng.randint(x_lo, hi)
    top = l2 - b - (l1 - x)                                 # c + l1 - x <= l2
    intron = rng.randint(want, min(top, want + 40)) if top >= want else rng.randint(6, top)
    c = b + intron
    contig[b:b + SLIDE] = contig[c:c + SLIDE]
    contig[c - SLIDE:c] = contig[b - SLIDE:b]
    contig = "".join(contig)
    return contig[b - x:b] + contig[c:c + l1 - x], contig


def dense_batch(rng, l1, l2, n, allowed=None, alpha="ACGT"):
    """n pairs of l1 x l2 and the dense list for them: (pairs, sites)"""
    allowed = allowed_columns(l2) if allowed is None else allowed
    sites = site_list(rng, l2, allowed)
    return [_pair(rng, l1, l2, allowed, k, alpha) for k in range(n)], sites


def dense_ragged(rng, r1, r2, n, lens1=None, spread=None, alpha="ACGT"):
    """n pairs with l1 in r1 (or drawn from lens1) and l2 in r2, l2 >= l1 + 20 (spread: l2 = l1 + 20 + one of these), under one dense
    list made for the longest l2: (pairs, sites)"""
    shapes = []
    for _ in range(n):
        l1 = rng.choice(lens1) if lens1 else rng.randint(*r1)
        l2 = l1 + 20 + rng.choice(spread) if spread else max(l1 + 20, rng.randint(*r2))
        shapes.append((l1, l2))
    max_l2 = max(s[1] for s in shapes)
    allowed = allowed_columns(max_l2)
    sites = site_list(rng, max_l2, allowed)
    return [_pair(rng, l1, l2, {a for a in allowed if a < l2}, k, alpha) for k, (l1, l2) in enumerate(shapes)], sites


# ---------------------------------------------------------------- oracle

_CACHE = {}


def _oracle(pairs, sc, uj, sites):
    """the restatement's result for every distinct pair, on at most 16 threads; computed once per (scoring, list) and pair"""
    memo = _CACHE.setdefault((sc, bool(uj), tuple(sites)), {})
    todo = [p for p in dict.fromkeys(pairs) if p not in memo]
    if todo:
        O.align(O.FIT, "A", "AA")                       # (loads the library before the threads start)
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            res = list(ex.map(lambda p: O.align(O.FIT, p[0], p[1], *sc, uj, sites), todo))
        memo.update(zip(todo, res))
    return memo


def _key(r, ops=True):
    return (r["score"], r["end_i"], r["end_j"], r["state"]) + ((r["ops"],) if ops else ())


def _has_jump(r):
    return O.OP_JUMP in r["ops"]


# ---------------------------------------------------------------- CPU half

# every (shape, scoring) the GPU half uses with reads of at most 150 bases: name -> (builder of (pairs, sites) for n pairs, scorings)
SENSITIVE = {
    "40x140": (lambda rng, n: dense_batch(rng, 40, 140, n), SCORINGS),     # (at 40 x 90 there is room for short introns only, which a gap
                                                                            # bridges as cheaply as a jump of -10: half the pairs jump)
    "60x140": (lambda rng, n: dense_batch(rng, 60, 140, n), SCORINGS),
    "150x500": (lambda rng, n: dense_batch(rng, 150, 500, n), SCORINGS),
    "150x500 ACGTN": (lambda rng, n: dense_batch(rng, 150, 500, n, alpha="ACGTN"), SCORINGS),
    "120x140": (lambda rng, n: dense_batch(rng, 120, 140, n), CHEAP),
    "ragged 105-128 x max(l1+20, 105-400)": (lambda rng, n: dense_ragged(rng, (105, 128), (105, 400), n), SCORINGS),
    "search 40-120 x 150-500": (lambda rng, n: _search_sets(rng, n, 1)[2:], SCORINGS[:1]),
}

def _search_sets(rng, nq, nt_per_q):
    """queries of 40 .. 120 bases spliced out of targets of 150 .. 500 under one dense list: (queries, targets, pairs, sites), pairs =
    every query with the target it came from"""
    allowed = allowed_columns(500)
    sites = site_list(rng, 500, allowed)
    queries, targets, pairs = [], [], []
    for k in range(nq):
        l1, l2 = rng.randint(40, 120), rng.randint(150, 500)
        q, t = _pair(rng, l1, l2, {a for a in allowed if a < l2}, k, unrelated_fourth=False)
        queries.append(q)
        targets.append(t)
        pairs.append((q, t))
        for _ in range(nt_per_q - 1):
            targets.append("".join(rng.choice("ACGT") for _ in range(rng.randint(150, 500))))
    return queries, targets, pairs, sites


@pytest.mark.parametrize("shape", list(SENSITIVE))
def test_batches_are_sensitive_to_the_list(shape):
    """A condition on the inputs: of a batch of 60, at least half of the pairs give another (score, end_j, state, ops) under the oracle
    with the list shifted by +1, at least half with it shifted by -1, at least half with the empty list.  A mask read one column off
    (or not at all) then fails most pairs of every batch instead of 3 of 200."""
    build, scorings = SENSITIVE[shape]
    pairs, sites = build(random.Random(zlib.crc32(shape.encode())), 60)
    for sc in scorings:
        ref = _oracle(pairs, sc, True, sites)
        shares = []
        for what, other in (("+1", [s + 1 for s in sites]), ("-1", [s - 1 for s in sites]), ("empty", [])):
            alt = _oracle(pairs, sc, True, other)
            changed = sum(1 for p in pairs if _key(ref[p]) != _key(alt[p]))
            shares.append(100 * changed // len(pairs))
            assert 2 * changed >= len(pairs), (shape, sc, what, changed, len(pairs))
        print("sensitivity %s %s: %d / %d / %d %% (+1 / -1 / empty), %d of %d with a jump" %
              (shape, sc, shares[0], shares[1], shares[2], sum(_has_jump(ref[p]) for p in pairs), len(pairs)))


def test_intron_classes_are_present():
    """at 150 x 500 the spliced reads hold introns of more than 64 and of more than 256 columns, and the oracle jumps over them"""
    pairs, sites = dense_batch(random.Random(5), 150, 500, 60)
    ref = _oracle(pairs, SCORINGS[0], True, sites)
    runs = [max((len(m) for m in re.findall(bytes([O.OP_JUMP]) + b"+", ref[p]["ops"])), default=0) for p in pairs]
    assert sum(r > 256 for r in runs) >= 5 and sum(64 < r <= 256 for r in runs) >= 5 and sum(0 < r <= 64 for r in runs) >= 5, sorted(runs)


@pytest.mark.parametrize("shape", [(40, 90), (150, 500), (300, 320)])
def test_oracle_all_columns_listed_is_no_jump(shape):
    """A list holding every column 0 .. l2 - 1 gives exactly the result of use_jump = False: score, end cell, state, ops"""
    l1, l2 = shape
    pairs, _ = dense_batch(random.Random(l1), l1, l2, 24)
    every = list(range(l2))
    for sc in SCORINGS:
        a = _oracle(pairs, sc, True, every)
        b = _oracle(pairs, sc, False, [])
        for p in pairs:
            assert _key(a[p]) == _key(b[p]) and (a[p]["r1"], a[p]["r2"]) == (b[p]["r1"], b[p]["r2"]), (shape, sc)


def test_oracle_values_outside_the_columns_are_the_empty_list():
    """A list holding only values < 0 or >= l2 gives the result of the empty list"""
    l1, l2 = 60, 140
    pairs, _ = dense_batch(random.Random(6), l1, l2, 24)
    outside = [-1, -2, -64, -65, INT32_MIN, l2, l2 + 1, l2 + 64, l2 + 191, INT32_MAX]
    for sc in SCORINGS:
        a = _oracle(pairs, sc, True, outside)
        b = _oracle(pairs, sc, True, [])
        assert sum(_has_jump(b[p]) for p in pairs) >= 8
        for p in pairs:
            assert _key(a[p]) == _key(b[p]), sc


@pytest.mark.skipif(not O.have_ref(), reason="compiled reference (oracle/_ref) not present")
def test_oracle_vs_live_reference_dense_lists():
    """The restatement against the compiled reference under dense, shuffled lists: random and spliced fit cases, l2 <= 120"""
    rng = random.Random(2718)
    n = jumps = 0
    for it in range(1500):
        l1 = rng.randint(1, 60)
        l2 = rng.randint(max(l1, 2), 120)
        allowed = allowed_columns(l2) if it % 3 else set(rng.sample(range(l2), min(l2, rng.randint(1, 6))))
        alpha = "ACGT"[:rng.randint(2, 4)]
        s1, s2 = _pair(rng, l1, l2, allowed, it, alpha)
        sites = site_list(rng, l2, allowed)
        sc = rng.choice(SCORINGS + [(1, -1, -1, -1, -3), (0, 0, 0, 0, 0)])
        a = O.align(O.FIT, s1, s2, *sc, True, sites)
        if a["rc"] == -2:
            continue
        b = O.ref_align(O.FIT, s1, s2, *sc, True, sites)
        assert (a["score"], a["r1"], a["r2"]) == (b["score"], b["r1"], b["r2"]), (it, sc, s1, s2)
        n += 1
        jumps += _has_jump(a)
    assert n > 1400 and jumps > 150, (n, jumps)


# ---------------------------------------------------------------- GPU half

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
    """monkeypatch with one chunk per host-entry call (a chunk on a helper handle would keep its own last_config)"""
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    for name in ("AT_TWO_PASS", "AT_TP_SPLIT", "AT_GROUP", "AT_STORE", "AT_NO_PACKED", "AT_WS_CAP_MB", "AT_WALK_TEAMS", "AT_CK_PIECE_PAIRS"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _compare(res, pairs, sc, uj, sites, tb, ctx):
    ref = _oracle(pairs, sc, uj, sites)
    for k, p in enumerate(pairs):
        r = ref[p]
        assert r["rc"] == 0, (ctx, k)
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]))
        assert got == _key(r, ops=False), (ctx, k, len(p[0]), len(p[1]))
        if tb:
            assert res["ops"][k] == r["ops"], (ctx, k, len(p[0]), len(p[1]))
    return ref


def _run(al, pairs, sc, sites, tb=True, ctx="", set_scoring=True):
    """align_batch (fit with the jump state) + every pair against the oracle.  Returns last_config."""
    if set_scoring:
        al.set_scoring(*sc, True, list(sites))
    res = al.align_batch("fit", pairs, traceback=tb, render=False)
    cfg = al.last_config
    _compare(res, pairs, sc, True, sites, tb, (ctx, sc, tb, cfg))
    return cfg


def _strings(al, pairs, sc, sites, ctx=""):
    """the two gapped strings rendered on the GPU against the oracle's r1 / r2 (a jump run renders like a U gap)"""
    al.set_scoring(*sc, True, list(sites))
    st = al.align_batch_strings("fit", pairs)
    cfg = al.last_config
    ref = _oracle(pairs, sc, True, sites)
    for k, p in enumerate(pairs):
        r = ref[p]
        assert (int(st["score"][k]), st["r1"][k], st["r2"][k]) == (r["score"], r["r1"], r["r2"]), (ctx, sc, k, cfg)
    return cfg


def _rep(uniq, n):
    """n pairs out of the distinct ones, repeated"""
    return [uniq[k % len(uniq)] for k in range(n)]


# family -> environment, builder of (pairs, sites), the scorings with the text at_last_config must hold for each.
# The scale: scores x16 (4-bit pointer cells, the jump pointers in the bit plane of AT_JPLANE) where 16 x the score range of
# packed_ok (at_hip.hip) stays inside 16 bits, else x4 (byte cells) on one 64-lane group, whatever the read length.
X16, X4 = "packed16 x16 ", "packed16 x4 "
FAMILIES = {
    "int32": (dict(AT_NO_PACKED="1"), lambda rng: dense_ragged(rng, (40, 200), (120, 300), 120),
              [(sc, ("int32",)) for sc in SCORINGS]),
    "g4": (dict(AT_TWO_PASS="0"), lambda rng: dense_batch(rng, 40, 140, 290),
           [(sc, (X16, "16x4-lane groups")) for sc in SCORINGS]),
    "g8": (dict(AT_TWO_PASS="0"), lambda rng: dense_batch(rng, 150, 500, 290),
           [(sc, (X16, "8x8-lane groups")) for sc in SCORINGS]),
    "g16": (dict(AT_TWO_PASS="0"), lambda rng: dense_batch(rng, 190, 220, 290),
            [(sc, (X16, "4x16-lane groups")) for sc in CHEAP]),
    "g32": (dict(AT_TWO_PASS="0", AT_GROUP="32"), lambda rng: dense_batch(rng, 350, 380, 250),
            [(CHEAP[0], (X16, "2x32-lane groups")), (CHEAP[1], (X4, "1x64-lane groups"))]),
    "g64": (dict(AT_TWO_PASS="0"), lambda rng: dense_batch(rng, 620, 660, 119),
            [(CHEAP[0], (X16, "1x64-lane groups")), (CHEAP[1], (X4, "1x64-lane groups"))]),
    "bytes": (dict(AT_TWO_PASS="0"), lambda rng: dense_batch(rng, 150, 500, 290, alpha="ACGTN"),
              [(sc, (X16, "bits=8", "8x8-lane groups")) for sc in SCORINGS]),
    "ragged 8-lane frames": ({}, lambda rng: dense_ragged(rng, (105, 128), (105, 400), 300),
                             [(sc, (X16, "8x8-lane groups", "ragged frames")) for sc in SCORINGS]),
    # (the shapes of test_ragged_long_reads_in_32_lane_frames, fitj: reads up to 416 bases; frames have no x4 form)
    "ragged 32-lane frames": ({}, lambda rng: dense_ragged(rng, None, None, 200, lens1=[305, 306, 319, 320, 321, 383, 384, 385, 415, 416] +
                                                           list(range(330, 416, 7)), spread=[0, 7, 90]),
                              [(CHEAP[0], (X16, "2x32-lane groups", "ragged frames"))]),
    "two-pass rounds 8-lane": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="0"), lambda rng: dense_batch(rng, 150, 500, 290),
                               [(sc, (X16, "8x8-lane groups", "two-pass ck=")) for sc in SCORINGS]),
    "walk kernel 8-lane": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="1"), lambda rng: dense_batch(rng, 150, 500, 290),
                           [(sc, (X16, "8x8-lane groups", "two-pass (walk kernel)")) for sc in SCORINGS]),
    "walk kernel 8-lane, teams": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="1", AT_WALK_TEAMS="1"), lambda rng: dense_batch(rng, 150, 500, 291),
                                  [(sc, (X16, "8x8-lane groups", "two-pass (walk kernel)")) for sc in SCORINGS[:2]]),
    "walk kernel 8-lane, pieces": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="1", AT_CK_PIECE_PAIRS="96"), lambda rng: dense_batch(rng, 150, 500, 291),
                                   [(sc, (X16, "two-pass (walk kernel)", "in pieces of")) for sc in SCORINGS[:2]]),
    "two-pass rounds 64-lane": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="0"), lambda rng: dense_batch(rng, 620, 660, 119),
                                [(CHEAP[0], (X16, "1x64-lane groups", "two-pass ck="))]),
    "walk kernel 64-lane": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="1"), lambda rng: dense_batch(rng, 620, 660, 119),
                            [(CHEAP[0], (X16, "1x64-lane groups", "two-pass (walk kernel)"))]),
    "walk kernel 64-lane, pieces": (dict(AT_TWO_PASS="2", AT_TP_SPLIT="1", AT_CK_PIECE_PAIRS="32"), lambda rng: dense_batch(rng, 620, 660, 119),
                                    [(CHEAP[0], (X16, "two-pass (walk kernel)", "in pieces of"))]),
}
TWO_PASS = ("two-pass rounds", "walk kernel")


def _family(env, family):
    knobs, build, cases = FAMILIES[family]
    for k, v in knobs.items():
        env.setenv(k, v)
    pairs, sites = build(random.Random(zlib.crc32(family.encode())))
    return pairs, sites, cases


def _check_cfg(cfg, family, want):
    for text in want:
        assert text in cfg, (family, text, cfg)
    if family.startswith("two-pass rounds"):
        assert "walk kernel" not in cfg, cfg
    elif not family.startswith("walk kernel"):
        assert "two-pass" not in cfg, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernel_family_under_dense_lists(al, env, family):
    """Every kernel family that reads the site mask, with tracebacks and scores only (the two-pass families: tracebacks are their
    subject): the 4- to 64-lane groups, both formats of the jump pointers (x16: bit plane, x4: byte cells), byte words, ragged frames
    of 8- and of 32-lane groups, the int32 kernel, the rounds inside the sweep's kernel and the walk kernel (one walker per half-lane,
    teams of lanes, batches in pieces) on the 8- and 64-lane groups."""
    pairs, sites, cases = _family(env, family)
    for sc, want in cases:
        for tb in ((True,) if family.startswith(TWO_PASS) else (True, False)):
            cfg = _run(al, pairs, sc, sites, tb=tb, ctx=family)
            if tb:
                _check_cfg(cfg, family, want)
            else:
                assert want[0] in cfg and "two-pass" not in cfg, (family, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_rendering_under_dense_lists(al, env, family):
    """Per family, one batch through align_batch_strings against the oracle's r1 / r2"""
    pairs, sites, cases = _family(env, family)
    sc, want = cases[0]
    cfg = _strings(al, pairs[:120], sc, sites, ctx=family)
    _check_cfg(cfg, family, [t for t in want if t != "in pieces of"])
    assert "[strings: " in cfg, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("store", [0, 1, 2])
def test_int32_storage_classes_under_dense_lists(al, env, store):
    """AT_NO_PACKED=1 with AT_STORE 0, 1 and 2: ragged batches, l1 40 .. 200, l2 120 .. 300 (scores only there is no pointer matrix,
    so store 1 is store 0: choose_store)"""
    env.setenv("AT_NO_PACKED", "1")
    env.setenv("AT_STORE", str(store))
    pairs, sites = dense_ragged(random.Random(20 + store), (40, 200), (120, 300), 120)
    for sc in SCORINGS:
        for tb in (True, False):
            cfg = _run(al, pairs, sc, sites, tb=tb, ctx=("int32", store))
            assert cfg.startswith("int32") and STORE_NAMES[store if tb or store != 1 else 0] in cfg, (store, tb, cfg)


@pytest.mark.gpu
def test_values_outside_int32_columns_are_skipped(al, env):
    """INT32_MIN and INT32_MAX in the list: ensure_sitemask skips them (no bit of theirs, no overflow of j + 65); same list to the oracle"""
    env.setenv("AT_TWO_PASS", "0")
    rng = random.Random(31)
    pairs, sites = dense_batch(rng, 150, 500, 120)
    sites = sites[:100] + [INT32_MAX, INT32_MIN] + sites[100:] + [INT32_MIN, INT32_MAX]
    for tb in (True, False):
        cfg = _run(al, pairs, SCORINGS[0], sites, tb=tb, ctx="INT32_MIN / INT32_MAX")
        assert X16 in cfg and "8x8-lane groups" in cfg, cfg
    env.setenv("AT_NO_PACKED", "1")
    assert _run(al, pairs[:40], SCORINGS[0], sites, ctx="INT32_MIN / INT32_MAX, int32").startswith("int32")


@pytest.mark.gpu
def test_sliver_as_32_lane_items_with_the_jump_state(al, env):
    """The construction of test_many_items_per_wave["sliver"] at 150 x 500 with the jump state: a cap on the workspace shrinks the grid
    to G waves, then three rounds of 8-lane items and one more item's worth, which goes to 32-lane items.  A deviation from that
    construction's AT_WS_CAP_MB=1: one pointer slot of this shape is about 0.6 MB, 1 MB leaves a grid of one wave, and the sliver rule
    needs four; the cap is the smallest number of MB that holds five slots, from the slot size a probe reports.  Scores only there is
    no pointer slot and the cap does not bind: that pass checks the results only."""
    env.setenv("AT_TWO_PASS", "0")
    rng = random.Random(41)
    uniq, sites = dense_batch(rng, 150, 500, 293)
    sc = SCORINGS[0]
    probe = _run(al, uniq[:40], sc, sites, ctx="probe")
    slot = int(re.search(r"slot=(\d+)B", probe).group(1))
    cap_mb = -(-5 * slot >> 20)
    g = (cap_mb << 20) // slot
    assert 5 <= g <= 16, probe
    env.setenv("AT_WS_CAP_MB", str(cap_mb))
    pairs = _rep(uniq, 16 * (3 * g + 1) - 7)
    for tb in (True, False):
        cfg = _run(al, pairs, sc, sites, tb=tb, ctx="sliver")
        assert "8x8-lane groups" in cfg, cfg
        if tb:
            assert _grid(cfg) == g and re.search(r"last 9 pairs as 32-lane items", cfg), cfg


def _grid(cfg):
    return int(re.search(r"grid=(\d+)", cfg).group(1))


@pytest.mark.gpu
def test_mask_lifetime_on_one_handle(al, env):
    """One handle, one at_set_scoring, batches of l2 = 90, then 500, then 90 again.  The list's allowed columns lie above 346, the bits
    the mask built for l2 = 90 does not hold: the second batch needs a mask rebuilt for its own l2 (sitemask_for_l2), and the third is
    served by the longer one."""
    import aligntools.c_amd as A
    rng = random.Random(51)
    allowed = {c for c in allowed_columns(500) if c > 346}
    assert len(allowed) >= 8
    long_pairs, sites = dense_batch(rng, 150, 500, 200, allowed)
    short_a = [_pair(rng, 40, 90, set(), k) for k in range(100)]
    short_b = [_pair(rng, 40, 90, set(), k) for k in range(64)]
    sc = SCORINGS[0]
    h = A.Aligner()
    try:
        h.set_scoring(*sc, True, sites)
        for name, pairs in (("first, l2 = 90", short_a), ("second, l2 = 500", long_pairs), ("third, l2 = 90", short_b), ("fourth, l2 = 500", long_pairs[::-1])):
            for tb in (True, False):
                cfg = _run(h, pairs, sc, sites, tb=tb, ctx=name, set_scoring=False)
                assert X16 in cfg, cfg
    finally:
        h.close()
    ref = _oracle(long_pairs, sc, True, sites)
    assert sum(_has_jump(ref[p]) for p in long_pairs) >= 50


@pytest.mark.gpu
def test_helper_handles_take_the_new_list(al, env):
    """Chunks side by side on helper handles (AT_HOST_CHUNK_MIN=64, 700 pairs of 120 x 140): list A, then set_scoring with list B of
    the same length, shifted by one, and the same pairs again -- every helper's mask is rebuilt"""
    env.delenv("AT_HOST_CHUNKS")
    env.setenv("AT_HOST_CHUNK_MIN", "64")
    rng = random.Random(61)
    uniq, a = dense_batch(rng, 120, 140, 233)
    pairs = _rep(uniq, 700)
    b = [s + 1 for s in a]
    sc = CHEAP[1]
    for name, sites in (("list A", a), ("list B", b), ("list A again", a)):
        cfg = _run(al, pairs, sc, sites, ctx=name)
        assert cfg.endswith(" x6 chunks"), cfg
    ra, rb = _oracle(uniq, sc, True, a), _oracle(uniq, sc, True, b)
    assert 2 * sum(_key(ra[p]) != _key(rb[p]) for p in uniq) >= len(uniq)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["int32", "g4", "g8", "g64", "two-pass rounds 8-lane", "walk kernel 8-lane", "walk kernel 64-lane"])
def test_all_columns_listed_equals_no_jump_on_the_device(al, env, family):
    """The list of every column 0 .. l2 - 1 against use_jump = False on the same pairs: every output equal"""
    pairs, _, cases = _family(env, family)
    sc, want = cases[0]
    l2 = max(len(b) for _, b in pairs)
    al.set_scoring(*sc, True, list(range(l2)))
    with_list = al.align_batch("fit", pairs, traceback=True, render=False)
    _check_cfg(al.last_config, family, want)
    al.set_scoring(*sc, False, [])
    without = al.align_batch("fit", pairs, traceback=True, render=False)
    for key in ("score", "end_i", "end_j", "state", "nops"):
        assert (np.asarray(with_list[key]) == np.asarray(without[key])).all(), (family, key)
    assert with_list["ops"] == without["ops"], family


@pytest.mark.gpu
def test_search_under_a_dense_list(al, env):
    """Aligner.search("fit", ...) with one dense list: queries of 40 .. 120 bases, targets of 150 .. 500, k = 5, against brute force
    over align_batch, and every hit's score, end cell and state against the oracle"""
    rng = random.Random(71)
    queries, targets, own, sites = _search_sets(rng, 24, 2)
    sc = SCORINGS[0]
    al.set_scoring(*sc, True, sites)
    nq, nt, k = len(queries), len(targets), 5
    allp = [(q, t) for q in queries for t in targets]
    res = al.align_batch("fit", allp, traceback=False, render=False)
    score = np.asarray(res["score"], dtype=np.int64).reshape(nq, nt)
    got = al.search("fit", queries, targets, k=k)
    assert al.last_config.startswith("search: "), al.last_config
    for q in range(nq):
        order = np.argsort(-score[q], kind="stable")[:k]         # ties keep the smaller target index
        assert int(got["nhits"][q]) == k
        assert [int(t) for t in got["target"][q]] == [int(t) for t in order], q
        hits = [(queries[q], targets[int(t)]) for t in order]
        ref = _oracle(hits, sc, True, sites)
        for h, p in enumerate(hits):
            have = tuple(int(got[name][q, h]) for name in ("score", "end_i", "end_j", "state"))
            assert have == _key(ref[p], ops=False), (q, h)
            t = int(order[h])
            assert have == tuple(int(res[name][q * nt + t]) for name in ("score", "end_i", "end_j", "state")), (q, h)
    ref = _oracle(own, sc, True, sites)
    assert sum(_has_jump(ref[p]) for p in own) >= nq // 2
