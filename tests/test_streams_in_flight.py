"""The device entries on real streams, with launches in flight (include/aligntools_hip.h: "use it with ONE stream at a time (calls queued
on the same stream may follow each other without waiting; a call on another stream needs the earlier ones finished -- or its own handle").

Every other file of the suite hands the device entries the null stream and waits after each call.  Here the calls are queued on
torch.cuda.Stream objects behind a GATE -- a spin kernel that keeps the stream busy while the host issues -- so that every launch of a
test is demonstrably queued behind work that has not finished: the work counter and the walkers' counters, the workspace slots, the
checkpoint buffer, the flag word of the device-side shape check, the scan scratch of the post-passes and the site mask are all handed
from one queued launch to the next.  A test asserts `not gate_event.query()` after its last call: if the host was held up anywhere, the
test fails instead of proving nothing.

What is compared: every buffer of a step, whole -- results, ops slots, rendered strings, CIGAR counts / statistics / words, compacted
ops and offsets -- bit for bit against the same call made ALONE (null stream, a handle that takes part in nothing else, a device-wide
wait before and after).  All outputs are pre-filled with sentinels (-7 / 0xEE) and carry 64 guard bytes, so a pair that a stale work
counter skipped shows as a sentinel and a write behind a buffer shows in its guard.  Every 16th pair of each recipe (all of them below 300
pairs) also goes against the oracle directly: score, end cell, state, ops and the two strings.

One process, one issuing thread, five handles.  test_comparator_notices (CPU) is the file's proof that `same` can fail.
"""
import copy
import itertools
import os
import random
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O

gpu = pytest.mark.gpu

I32_FILL, U8_FILL, GUARD = -7, 0xEE, 64
FIELDS = ("score", "end_i", "end_j", "state", "nops")
DEFAULT = (1, -2, -5, -1, -10)
C3_SCORING = (1, -1, -4, -1, -10)       # bench.py's global 1 024 x 1 024 workload: scores x4 on the 64-lane groups
EDIT_SCORING = (0, 1, 0, 0, 0)          # the bit-parallel kernels need the unit mismatch cost
CHUNK = 10000                           # R9: pairs per slice of the triangle
MAX_GATE = 2.0


def _fill(dt):
    return U8_FILL if np.dtype(dt) == np.uint8 else I32_FILL


def _guard(dt):
    return GUARD // np.dtype(dt).itemsize


# ---------------------------------------------------------------- pairs

def _uniform_pairs(l1, l2, n, seed, related=True, windows=False):
    """n pairs of l1 x l2 as bytes; related: every odd s2 is a substituted copy of its s1; windows: every even s1 is a mutated window
    of its s2 (the fit -s input of bench.py)"""
    from aligntools.c_amd import synth as S
    blob = S.workload_blob("fit", True, seed, n, l1, l2) if windows else S.synth_pairs_blob(seed, n, l1, l2)
    if related and not windows:
        rel = S.mutate_pairs(blob, l1, l2, seed & 0xffff, sub=0.06)
        blob = np.where((np.arange(n) % 2 == 1)[:, None], rel, blob)
    rows, w = np.ascontiguousarray(blob).tobytes(), l1 + l2
    return [(rows[k * w:k * w + l1], rows[k * w + l1:(k + 1) * w]) for k in range(n)]


def _ragged_pairs(n, lo1, hi1, lo2, hi2, seed):
    rng = random.Random(seed)
    full = _uniform_pairs(hi1, hi2, n, seed)
    out = [(a[:rng.randint(lo1, hi1)], b[:rng.randint(lo2, hi2)]) for a, b in full]
    out[0] = full[0]                    # (the frame's own shape is in the batch)
    return out


# ---------------------------------------------------------------- recipes

class Recipe:
    """A named batch: mode, scoring, pairs, the call to make and what its last_config must say.  It stages its own device inputs
    (A.pack_pairs) and owns its output sets; no step shares one."""

    def __init__(self, name, mode, pairs, sc=DEFAULT, use_jump=False, sites=(), uniform=True, tb=True, cfg=(), cfg_not=(), env=None,
                 edit_tb=False, kind="batch"):
        self.name, self.mode, self.pairs, self.sc, self.use_jump, self.sites = name, mode, pairs, tuple(sc), bool(use_jump), tuple(sites)
        self.uniform, self.tb, self.cfg, self.cfg_not, self.env = bool(uniform), bool(tb), tuple(cfg), tuple(cfg_not), dict(env or {})
        self.edit_tb, self.kind = bool(edit_tb), kind
        self.max1 = max(len(a) for a, _ in pairs)
        self.max2 = max(len(b) for _, b in pairs)
        if kind == "allpairs":
            self.nreads = len(pairs)
            self.npairs = self.nreads * (self.nreads - 1) // 2
            self.nslices = (self.npairs + CHUNK - 1) // CHUNK
            self.n, self.slot = self.npairs, 0          # (outputs are indexed by the pair's place in the triangle)
            self.lay = {"res": (np.int32, 5 * CHUNK), "keep": (np.int32, self.nslices * 5 * CHUNK)}
        else:
            self.n = len(pairs)
            self.slot = self.max1 + self.max2
            self.cigar_cap = self.n * self.slot if self.n * self.slot <= (4 << 20) else self.n * 64
            self.lay = _layout(self.n, self.slot, self.tb, self.cigar_cap)
        self.dev = None
        self.sets = {}
        self.alone = None
        self._sample = None

    # ---- what the launches align, by output index
    def aligned_pair(self, k):
        if self.kind == "allpairs":
            a, b = self._tri[k]
            return self.pairs[a][0], self.pairs[b][0]
        if self.kind == "revcomp":
            import aligntools.c_amd as A
            return A.revcomp(self.pairs[k][0]), self.pairs[k][1]
        return self.pairs[k]

    def sample(self):
        """[(k, oracle result)] for every 16th pair, for all below 300 pairs; computed once"""
        if self._sample is None:
            if self.kind == "allpairs":
                self._tri = list(itertools.combinations(range(self.nreads), 2))   # (row-major strict upper triangle)
            ks = list(range(self.n)) if self.n < 300 else list(range(0, self.n, 16))
            mode = O.MODE_NAMES[self.mode]
            O.align(O.LOCAL, b"A", b"AA")               # (loads the library before the threads start)

            def one(k):
                a, b = self.aligned_pair(k)
                return O.align(mode, a, b, *self.sc, self.use_jump, list(self.sites))
            with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
                self._sample = list(zip(ks, ex.map(one, ks)))
            assert all(r["rc"] == 0 for _, r in self._sample), self.name
        return self._sample

    # ---- device side
    def stage(self, dev):
        if self.dev is not None:
            return
        import torch
        import aligntools.c_amd as A
        words, woff1, woff2, len1, len2, bits = A.pack_pairs(self.pairs, bits=2)
        assert bits == 2
        self.bits = bits
        d = dict(words=torch.from_numpy(words.view(np.int32)).to(dev))
        for key, v in (("woff1", woff1), ("woff2", woff2), ("len1", len1), ("len2", len2)):
            d[key] = torch.from_numpy(v).to(dev)
        if self.kind != "allpairs":
            d["ops_off"] = torch.arange(self.n, dtype=torch.int64, device=dev) * self.slot
        if self.kind == "revcomp":
            # the second word buffer starts as the first with every s1's words (and slack word) overwritten: a reverse complement that
            # is skipped, or that the sweep does not wait for, leaves words that are not the reads'
            init = words.view(np.int32).copy()
            nw = (len1.astype(np.int64) + 15) // 16 + 1
            for k in range(self.n):
                init[woff1[k]:woff1[k] + nw[k]] = 0x2EEEEEEE
            self.rc_init = torch.from_numpy(init).to(dev)
            self.lay["rc_words"] = (np.int32, int(init.size))
        self.dev = d

    def outputs(self, i, dev):
        """the i-th output set of this recipe (made and filled on first use)"""
        self.stage(dev)
        if i not in self.sets:
            self.sets[i] = Outputs(self, dev)
        return self.sets[i]


def _layout(n, slot, tb, cigar_cap):
    """name -> (dtype, elements in front of the 64 guard bytes)"""
    lay = {"res": (np.int32, 5 * n)}
    if tb:
        lay["ops"] = (np.uint8, n * slot)
        lay["r1"] = (np.uint8, n * slot)
        lay["r2"] = (np.uint8, n * slot)
        for f in ("x", "m"):                            # '=' / 'X', and AT_CIGAR_M
            lay["ncigar_" + f] = (np.int32, n)
            lay["stats_" + f] = (np.int32, 8 * n)
            lay["cigar_off_" + f] = (np.int64, n + 1)
            lay["cigar_" + f] = (np.int32, cigar_cap)
        lay["packed"] = (np.uint8, n * slot)
        lay["packed_off"] = (np.int64, n + 1)
    return lay


class Outputs:
    """One step's device buffers, every one pre-filled with its sentinel and 64 guard bytes behind it."""

    def __init__(self, recipe, dev):
        import torch
        tt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}
        self.r = recipe
        self.t = {name: torch.empty(elems + _guard(dt), dtype=tt[np.dtype(dt)], device=dev) for name, (dt, elems) in recipe.lay.items()}
        self.refill()

    def refill(self):
        import torch
        for t in self.t.values():
            t.fill_(U8_FILL if t.dtype == torch.uint8 else I32_FILL)
        if self.r.kind == "revcomp":
            self.t["rc_words"][:self.r.rc_init.numel()].copy_(self.r.rc_init)

    def ptr(self, name, elem=0):
        t = self.t[name]
        return t.data_ptr() + elem * t.element_size()

    def host(self, names=None):
        r = self.r
        out = dict(name=r.name, n=r.n, slot=r.slot, kind=r.kind, mode=r.mode, tb=r.tb, lay=r.lay)
        for name, t in self.t.items():
            if names is None or name in names:
                out[name] = t.cpu().numpy()
        return out


def make(name, grid, seed=0):
    """The recipes of one row of the table (R8 is two).  grid: the resident waves of the 8-lane local kernel (a probe launch's grid=)."""
    key = (name, grid, seed)
    if key not in _MADE:
        _MADE[key] = _make(name, grid, seed)
    return _MADE[key]


_MADE = {}
FIT_CFG = ("packed16 x16 bits=2 8x8-lane groups (16 pairs/wave)", "two-pass (walk kernel)")
LOCAL_CFG = ("packed16 x16 bits=2 8x8-lane groups (16 pairs/wave)",)


def _make(name, grid, seed):
    s = 0x51A0 + 977 * seed
    if name in ("R1", "R10"):
        # a whole round for every resident wave and an eighth more: waves pull a second item from the work counter, and the last round,
        # less than a quarter full, goes to the sliver's 32-lane items in the same launch
        n = 16 * (grid + grid // 8)
        pairs = make("R1", grid, seed)[0].pairs if name == "R10" else _uniform_pairs(150, 150, n, s + 1)
        return [Recipe(name, "local", pairs, cfg=LOCAL_CFG + ("as 32-lane items",), cfg_not=("two-pass",), kind="revcomp" if name == "R10" else "batch")]
    if name == "R2":
        return [Recipe("R2", "global", _uniform_pairs(700, 700, 96, s + 2), sc=C3_SCORING, env={"AT_PACKED_MIN_ROUNDS": "0"},
                       cfg=("packed16 x4 bits=2 1x64-lane groups (2 pairs/wave)", "two-pass (walk kernel)", "wavefronts of teams"))]
    if name == "R3":
        return [Recipe("R3", "fit", _uniform_pairs(150, 500, 1500, s + 3, windows=True), use_jump=True, sites=(100, 200, 300, 400), cfg=FIT_CFG)]
    if name == "R4":
        return [Recipe("R4", "fit", _uniform_pairs(150, 500, 1500, s + 4, windows=True), sc=(1, -2, -5, -1, -7), use_jump=True,
                       sites=(0, 17, 250, 499), cfg=FIT_CFG)]
    if name in ("R5", "R6"):
        pairs = _uniform_pairs(150, 150, 4200, s + 5)
        if name == "R6":
            pairs[4199] = (pairs[4199][0][:149], pairs[4199][1])
        return [Recipe(name, "local", pairs, uniform=False, cfg=("auto: [packed16 x16 bits=2 8x8-lane groups", "if every pair is 150x150, else [int32 bits=2"))]
    if name == "R7":
        return [Recipe("R7", "global", _uniform_pairs(300, 5000, 40, s + 7, related=False), cfg=("int32 bits=2",), cfg_not=("packed16", "auto:"))]
    if name == "R8":
        return [Recipe("R8a", "edit", _ragged_pairs(3000, 257, 400, 200, 420, s + 8), sc=EDIT_SCORING, uniform=False, tb=False,
                       cfg=("myers bits=2",)),
                Recipe("R8b", "edit", _uniform_pairs(150, 150, 1000, s + 9), sc=EDIT_SCORING, edit_tb=True, cfg=("myers-tb bits=2",))]
    if name == "R9":
        reads = [(a, b"") for a, _ in _uniform_pairs(100, 4, 300, s + 10, related=False)]
        half = reads[0][0][:50]
        for k in range(1, 300, 3):                      # (real overlaps: every third read begins with the first one's first half)
            reads[k] = (half + reads[k][0][50:], b"")
        return [Recipe("R9", "overlap", reads, tb=False, uniform=False, cfg=("int32 bits=2",), cfg_not=("overlap filter",), kind="allpairs")]
    raise KeyError(name)


TABLE = ("R1", "R2", "R3", "R4", "R5", "R6", "R7", "R8", "R9", "R10")


# ---------------------------------------------------------------- issuing

def issue(r, h, outs, ts, env, post=True):
    """Queue recipe r on handle h and torch stream ts into the output set `outs`: the alignment and, with tracebacks, the three
    post-passes behind it on the same stream.  No host wait."""
    import torch
    import aligntools.c_amd as A
    s, d, n = ts.cuda_stream, r.dev, r.n
    h.set_scoring(*r.sc, r.use_jump, list(r.sites))
    h.set_edit_traceback(r.edit_tb)
    for k, v in r.env.items():
        env.setenv(k, v)
    try:
        if r.kind == "allpairs":
            row = lambda i: outs.ptr("res", i * CHUNK)
            for i, first in enumerate(range(0, r.npairs, CHUNK)):
                h.align_allpairs_device(A.MODES[r.mode], r.nreads, d["words"].data_ptr(), r.bits, d["woff1"].data_ptr(), d["len1"].data_ptr(),
                                        r.max1, first, min(CHUNK, r.npairs - first), False, row(0), row(1), row(2), row(3), None, None, None, s)
                _says(r, h)
                with torch.cuda.stream(ts):             # (every slice is copied away before the next one overwrites it)
                    outs.t["keep"][i * 5 * CHUNK:(i + 1) * 5 * CHUNK].copy_(outs.t["res"][:5 * CHUNK])
            return
        words = d["words"].data_ptr()
        if r.kind == "revcomp":                         # the sweep reads what the launch before it wrote
            words = outs.ptr("rc_words")
            h.revcomp_device(n, d["words"].data_ptr(), r.bits, d["woff1"].data_ptr(), d["len1"].data_ptr(), words, None, s)
        row = lambda i: outs.ptr("res", i * n)
        tb = r.tb
        h.align_batch_device(A.MODES[r.mode], n, words, r.bits, d["woff1"].data_ptr(), d["len1"].data_ptr(), d["woff2"].data_ptr(),
                             d["len2"].data_ptr(), r.max1, r.max2, r.uniform, tb, row(0), row(1), row(2), row(3),
                             outs.ptr("ops") if tb else None, d["ops_off"].data_ptr() if tb else None, row(4) if tb else None, s)
        _says(r, h)
    finally:
        for k in r.env:
            env.delenv(k, raising=False)
    if not (tb and post):
        return
    common = (words, r.bits, d["woff1"].data_ptr(), d["woff2"].data_ptr(), row(1), row(2), outs.ptr("ops"), d["ops_off"].data_ptr(), row(4))
    h.render_batch_device(n, *common, outs.ptr("r1"), outs.ptr("r2"), None, False, s)
    for f, ext in (("m", False), ("x", True)):
        h.cigar_batch_device(n, *common, outs.ptr("ncigar_" + f), outs.ptr("stats_" + f), outs.ptr("cigar_off_" + f), outs.ptr("cigar_" + f),
                             r.cigar_cap, extended=ext, stream=s)
    h.compact_ops_device(n, outs.ptr("ops"), d["ops_off"].data_ptr(), row(4), outs.ptr("packed"), n * r.slot, outs.ptr("packed_off"), s)


_SAID = {}                              # recipe -> the last_config of its latest launch (printed by the first test)


def _says(r, h):
    cfg = _SAID[r.name] = h.last_config
    assert all(x in cfg for x in r.cfg) and not any(x in cfg for x in r.cfg_not), (r.name, r.cfg, r.cfg_not, cfg)


def run_alone(r, rig, env):
    """The same call on the null stream of a handle that takes part in nothing else, a device-wide wait before and after.  Host copies,
    made once per recipe."""
    import torch
    if r.alone is None:
        outs = r.outputs("alone", rig.dev)
        torch.cuda.synchronize()
        issue(r, rig.handle(0), outs, torch.cuda.default_stream(), env)
        torch.cuda.synchronize()
        r.alone = outs.host()
        del r.sets["alone"]
    return r.alone


# ---------------------------------------------------------------- the comparator

def same(got, alone, oracle_sample, only=None):
    """got == alone, every buffer whole (guards and untouched bytes included), and the sampled pairs against the oracle."""
    name, n, slot, lay = alone["name"], alone["n"], alone["slot"], alone["lay"]
    names = [x for x in lay if only is None or x in only]
    batch = alone["kind"] != "allpairs"
    if batch:
        res = got["res"][:5 * n].reshape(5, n)
        never = np.flatnonzero((res[:4] == I32_FILL).all(axis=0))
        assert never.size == 0, "%s: pair %d was never written (all of its results are the sentinel)" % (name, int(never[0]))
    for x in names:
        dt, elems = lay[x]
        g, a = got[x], alone[x]
        assert g.dtype == a.dtype and g.shape == a.shape == (elems + _guard(dt),), (name, x, g.shape, a.shape)
        for who, arr in (("in flight", g), ("alone", a)):
            hit = np.flatnonzero(arr[elems:] != _fill(dt))
            assert hit.size == 0, "%s: %s, %s: guard byte changed at element %d behind the buffer" % (name, x, who, int(hit[0]))
        bad = np.flatnonzero(g[:elems] != a[:elems])
        if bad.size:
            at = int(bad[0])
            what = "%s of pair %d" % (FIELDS[at // n], at % n) if x == "res" and batch else "element %d" % at
            if x in ("ops", "r1", "r2") and slot:
                what += " (pair %d, byte %d of its slot)" % (at // slot, at % slot)
            raise AssertionError("%s: %s differs from the run alone at %s: %r != %r (%d differences)" % (name, x, what, g[at], a[at], bad.size))
    if batch and alone["tb"] and (only is None or "packed_off" in only):
        # (every pair's words and bytes were inside the capacities, so all of them were compared)
        assert 0 <= alone["packed_off"][n] <= lay["packed"][1], (name, int(alone["packed_off"][n]))
        if only is None:
            for f in ("x", "m"):
                assert 0 <= alone["cigar_off_" + f][n] <= lay["cigar_" + f][1], (name, f, int(alone["cigar_off_" + f][n]))
    for k, ref in oracle_sample or ():
        if not batch:
            i, off = divmod(k, CHUNK)
            keep = got["keep"]
            assert int(keep[(5 * i) * CHUNK + off]) == ref["score"], (name, "pair %d against the oracle" % k)
            continue
        r5 = tuple(int(v) for v in res[:, k])
        if alone["mode"] == "edit":
            assert r5[0] == ref["score"], (name, "pair %d against the oracle" % k, r5, ref["score"])
            continue
        want = (ref["score"], ref["end_i"], ref["end_j"])
        assert r5[:3] == want, (name, "pair %d against the oracle" % k, r5, want)
        if alone["tb"]:
            assert (r5[3], r5[4]) == (ref["state"], len(ref["ops"])), (name, "pair %d against the oracle" % k, r5)
            o = k * slot
            assert got["ops"][o:o + r5[4]].tobytes() == ref["ops"], (name, "ops of pair %d against the oracle" % k)
            if "r1" in names:
                assert got["r1"][o:o + r5[4]].tobytes().decode("latin1") == ref["r1"], (name, "r1 of pair %d against the oracle" % k)
                assert got["r2"][o:o + r5[4]].tobytes().decode("latin1") == ref["r2"], (name, "r2 of pair %d against the oracle" % k)


def _hand_made():
    """a small alone copy made by hand: 4 pairs, slots of 8 bytes, with tracebacks and post-passes"""
    n, slot = 4, 8
    lay = _layout(n, slot, True, n * slot)
    h = dict(name="hand", n=n, slot=slot, kind="batch", mode="local", tb=True, lay=lay)
    for x, (dt, elems) in lay.items():
        h[x] = np.full(elems + _guard(dt), _fill(dt), dtype=dt)
    nops = np.array([3, 0, 8, 5], dtype=np.int32)
    res = h["res"][:5 * n].reshape(5, n)
    res[0], res[1], res[2], res[3], res[4] = [12, 0, -3, 7], [5, 1, 8, 6], [4, 1, 8, 7], [2, 2, 2, 2], nops
    off = np.concatenate(([0], np.cumsum(nops))).astype(np.int64)
    for k in range(n):
        ops = (np.arange(nops[k]) % 3).astype(np.uint8)
        h["ops"][k * slot:k * slot + nops[k]] = ops
        h["r1"][k * slot:k * slot + nops[k]] = 65
        h["r2"][k * slot:k * slot + nops[k]] = 67
        h["packed"][off[k]:off[k + 1]] = ops
    h["packed_off"][:n + 1] = off
    for f in ("x", "m"):
        h["ncigar_" + f][:n] = [1, 0, 2, 1]
        h["stats_" + f][:8 * n] = np.arange(8 * n)
        h["cigar_off_" + f][:n + 1] = [0, 1, 1, 3, 4]
        h["cigar_" + f][:4] = [(3 << 4) | 7, (6 << 4) | 7, (2 << 4) | 8, (5 << 4) | 0]
    return h


def test_comparator_notices():
    alone = _hand_made()
    n, slot = alone["n"], alone["slot"]
    same(copy.deepcopy(alone), alone, None)             # (an exact copy passes)

    def wrong_score(g):
        g["res"][0 * n + 2] += 1

    def left_at_sentinel(g):
        for i in range(5):
            g["res"][i * n + 3] = I32_FILL
        g["ops"][3 * slot:4 * slot] = U8_FILL

    def op_below_nops(g):
        g["ops"][2 * slot + 7] ^= 1                     # (pair 2 has 8 ops: its last one)

    def guard_byte(g):
        g["r2"][n * slot + 63] = 0

    def cigar_word(g):
        g["cigar_x"][2] += 16

    def compacted_offset(g):
        g["packed_off"][2] += 1

    for case in (wrong_score, left_at_sentinel, op_below_nops, guard_byte, cigar_word, compacted_offset):
        g = copy.deepcopy(alone)
        case(g)
        with pytest.raises(AssertionError):
            same(g, alone, None)
        changed = sum(int((g[x] != alone[x]).sum()) for x in alone["lay"])
        assert changed == (1 if case is not left_at_sentinel else 5 + 5), (case.__name__, changed)
    # ... and the oracle half: a result that equals the alone copy but not the oracle
    ref = dict(score=12, end_i=5, end_j=4, state=2, ops=bytes([0, 1, 2]), r1="AAA", r2="CCC")
    same(copy.deepcopy(alone), alone, [(0, ref)])
    for key, v in (("score", 11), ("end_j", 5), ("ops", bytes([0, 1, 1])), ("r2", "CCG")):
        with pytest.raises(AssertionError):
            same(copy.deepcopy(alone), alone, [(0, dict(ref, **{key: v}))])


def test_recipes_lie_in_the_oracles_domain():
    """every recipe's sampled pairs give rc == 0 in the oracle (with a small stand-in for the card's grid)"""
    for name in TABLE:
        for r in make(name, 8, seed=1):
            assert r.sample() and all(ref["rc"] == 0 for _, ref in r.sample()), r.name
    R6 = make("R6", 8, seed=1)[0]
    assert (len(R6.pairs[4199][0]), len(R6.pairs[4199][1])) == (149, 150) and R6.max1 == 150


# ---------------------------------------------------------------- the rig

class Rig:
    """The file's five handles (0: the one that runs alone), four streams, the gate's calibration and the probe launch's grid."""

    def __init__(self):
        import torch
        self.dev = torch.device("cuda", 0)
        self.handles = {}
        self.used = set()
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(4)]
        # cycles per second of torch.cuda._sleep's clock: one call between two timing events
        torch.cuda._sleep(100000)
        torch.cuda.synchronize()
        cycles = 2000000
        for _ in range(2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0:
                break
            cycles *= 20                                # (a fast clock: a longer spin, so that the launch itself does not count)
        self.cycles_per_s = cycles / (ms / 1e3)
        self.grid = self._probe()

    def handle(self, i):
        import aligntools.c_amd as A
        assert 0 <= i < 5
        if i not in self.handles:
            self.handles[i] = A.Aligner(0)
        self.used.add(i)
        return self.handles[i]

    def fresh(self, i):
        """handle i, never used before (made anew if an earlier test has used it)"""
        if i in self.used:
            self.handles.pop(i).close()
            self.used.discard(i)
        return self.handle(i)

    def _probe(self):
        """grid= of a local 150 x 150 launch large enough to fill the card: the resident waves of R1's kernel"""
        import torch
        import aligntools.c_amd as A
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        n, w = 16 * 16 * ncu, 11
        words = torch.zeros(n * 2 * w + 4, dtype=torch.int32, device=self.dev)
        woff1 = torch.arange(n, dtype=torch.int64, device=self.dev) * (2 * w)
        woff2 = woff1 + w
        lens = torch.full((n,), 150, dtype=torch.int32, device=self.dev)
        res = torch.zeros((5, n), dtype=torch.int32, device=self.dev)
        ops = torch.zeros(n * 300 + 64, dtype=torch.uint8, device=self.dev)
        ops_off = torch.arange(n, dtype=torch.int64, device=self.dev) * 300
        h = self.handle(0)
        h.set_scoring(*DEFAULT)
        h.align_batch_device(A.MODE_LOCAL, n, words.data_ptr(), 2, woff1.data_ptr(), lens.data_ptr(), woff2.data_ptr(), lens.data_ptr(), 150, 150,
                             True, True, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), ops.data_ptr(),
                             ops_off.data_ptr(), res[4].data_ptr(), 0)
        torch.cuda.synchronize()
        m = re.search(r"grid=(\d+)", h.last_config)
        assert m and LOCAL_CFG[0] in h.last_config, h.last_config
        return int(m.group(1))

    def gate(self, ts, seconds):
        """a spin of about `seconds` on ts; returns an event recorded right behind it"""
        import torch
        with torch.cuda.stream(ts):
            torch.cuda._sleep(int(seconds * self.cycles_per_s))
        ev = torch.cuda.Event()
        ev.record(ts)
        return ev

    def gate_length(self, t_issue):
        g = max(4.0 * t_issue, 0.05)                    # (the factor 4: the spread of host issue time on a shared machine)
        assert g <= MAX_GATE, "issuing is too slow: %.3f s for the queue, a gate of %.3f s would exceed %.1f s" % (t_issue, g, MAX_GATE)
        return g

    def close(self):
        import torch
        torch.cuda.synchronize()
        for h in self.handles.values():
            h.close()
        self.handles.clear()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()
    _MADE.clear()


def _refill(steps):
    import torch
    for _, outs in steps:
        outs.refill()
    torch.cuda.synchronize()


def _compare(steps, rig, env, only=None):
    for r, outs in steps:
        same(outs.host(), run_alone(r, rig, env), r.sample(), only)


def _report(record_property, **kv):
    for k, v in kv.items():
        record_property(k, v)
    print("\n[streams in flight] " + ", ".join("%s=%s" % (k, ("%.4f" % v) if isinstance(v, float) else v) for k, v in kv.items()))


# ---------------------------------------------------------------- the tests

@gpu
def test_queue_on_one_stream_behind_a_gate(rig, monkeypatch, record_property):
    """One handle, one stream, the whole table queued twice (listed order, then reversed) behind a gate: every launch is issued while the
    stream still holds the gate, so each one inherits the handle's counters, workspace, checkpoints, flag word, scan scratch and site
    mask from a launch that has not run yet."""
    import torch
    h, ts = rig.handle(1), rig.streams[0]
    order = [r for name in TABLE for r in make(name, rig.grid)]
    for r in order:
        run_alone(r, rig, monkeypatch)
    queue = [(r, r.outputs(0, rig.dev)) for r in order] + [(r, r.outputs(1, rig.dev)) for r in reversed(order)]
    torch.cuda.synchronize()
    for r, outs in queue[:len(order)]:                 # warm-up: the grow-only buffers reach their size (R4 and R7 in the rehearsal)
        if r.name not in ("R4", "R7"):
            issue(r, h, outs, ts, monkeypatch)
            ts.synchronize()
    t0 = time.perf_counter()                            # rehearsal: how long does the host take to issue the queue?
    for r, outs in queue:
        issue(r, h, outs, ts, monkeypatch)
    t_issue = time.perf_counter() - t0
    ts.synchronize()
    gate_s = rig.gate_length(t_issue)
    _refill(queue)
    ev = rig.gate(ts, gate_s)
    for r, outs in queue:
        issue(r, h, outs, ts, monkeypatch)
    held = not ev.query()
    ts.synchronize()
    _report(record_property, test1_t_issue_s=t_issue, test1_gate_s=gate_s, test1_steps=len(queue), grid=rig.grid,
            pairs=str({r.name: r.n for r in order}))
    print("\n".join("  %-4s %s" % kv for kv in _SAID.items()))
    assert held, "the gate (%.3f s) opened before the last call was issued (rehearsal: %.4f s): some call waited for the device" % (gate_s, t_issue)
    _compare(queue, rig, monkeypatch)


@gpu
def test_growth_and_scoring_changes_between_queued_launches(rig, monkeypatch):
    """A fresh handle, no warm-up, no gate: workspace, checkpoint buffer and site mask grow or change behind a launch just queued.  The
    library waits by design here (grow()'s hipFree waits for the device before a buffer that a queued launch may still use goes away),
    so this test checks correctness, not overlap.  Then the same handle on a second stream, after the first has been waited for: the
    contract's "a call on another stream needs the earlier ones finished".

    R8b stands in front of the order R1, R3, R4, R2, R7, R8, R3: R1's workspace (the pointer slots of every resident wave, 400 MB on a
    card of 256 CUs) is the largest of the table, R7's 40 slots of 1.3 MB included, so behind R1 the workspace never grows again.  With
    R8b's 6 MB slab first, R1's launch frees a workspace that the launch queued just before it is using."""
    h, ts, ts2 = rig.fresh(4), rig.streams[0], rig.streams[1]
    g = rig.grid
    recipes = make("R8", g)[1:] + make("R1", g) + make("R3", g) + make("R4", g) + make("R2", g) + make("R7", g) + make("R8", g) + make("R3", g)
    seen, steps = {}, []
    for r in recipes:
        i = seen[r.name] = seen.get(r.name, -1) + 1
        steps.append((r, r.outputs(i, rig.dev)))
    _refill(steps)
    for r, outs in steps:
        issue(r, h, outs, ts, monkeypatch)
    ts.synchronize()
    _compare(steps, rig, monkeypatch)
    again = [(r, r.outputs(1, rig.dev)) for r in make("R1", g) + make("R2", g)]
    _refill(again)
    for r, outs in again:
        issue(r, h, outs, ts2, monkeypatch)
    ts2.synchronize()
    _compare(again, rig, monkeypatch)


@gpu
def test_three_handles_three_streams(rig, monkeypatch, record_property):
    """bench.py's pattern: twelve steps, step k on streams[k % 3] with handles[k % 3], every step with pairs and buffers of its own,
    all issued behind a gate on every stream."""
    import torch
    hs, tss = [rig.handle(i) for i in (1, 2, 3)], rig.streams[:3]
    cycle = ("R1", "R2", "R3", "R5", "R8")
    steps = []
    for k in range(12):
        for r in make(cycle[k % 5], rig.grid, seed=100 + k):
            run_alone(r, rig, monkeypatch)
            steps.append((k, r, r.outputs(0, rig.dev)))
    pairs_of = [(r, outs) for _, r, outs in steps]
    torch.cuda.synchronize()
    for k, r, outs in steps:                            # warm-up
        issue(r, hs[k % 3], outs, tss[k % 3], monkeypatch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()                            # rehearsal
    for k, r, outs in steps:
        issue(r, hs[k % 3], outs, tss[k % 3], monkeypatch)
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    gate_s = rig.gate_length(t_issue)
    _refill(pairs_of)
    base = torch.cuda.Event(enable_timing=True)
    base.record()
    base.synchronize()
    first = [torch.cuda.Event(enable_timing=True) for _ in tss]
    last = [torch.cuda.Event(enable_timing=True) for _ in tss]
    gates = [rig.gate(ts, gate_s) for ts in tss]
    for ev, ts in zip(first, tss):
        ev.record(ts)
    for k, r, outs in steps:
        issue(r, hs[k % 3], outs, tss[k % 3], monkeypatch)
    for ev, ts in zip(last, tss):
        ev.record(ts)
    held = [not ev.query() for ev in gates]
    torch.cuda.synchronize()
    spans = [(base.elapsed_time(a), base.elapsed_time(b)) for a, b in zip(first, last)]
    intersect = max(a for a, _ in spans) < min(b for _, b in spans)
    _report(record_property, test3_t_issue_s=t_issue, test3_gate_s=gate_s, test3_intervals_ms=str([(round(a, 3), round(b, 3)) for a, b in spans]),
            test3_intervals_intersect=bool(intersect))    # (reported, not asserted: how the card interleaves its queues is not the library's contract)
    assert all(held), "a gate (%.3f s) opened before the last call was issued (rehearsal: %.4f s): %s" % (gate_s, t_issue, held)
    _compare(pairs_of, rig, monkeypatch)


@gpu
def test_consumer_on_another_stream_behind_events(rig, monkeypatch, record_property):
    """As bench.py's gather: another handle on another stream compacts the ops of two producers' steps, each waited for with
    wait_event(ev) and nothing else; the producers are gated."""
    import torch
    prod = [(rig.handle(1), rig.streams[0], make("R1", rig.grid)[0]), (rig.handle(2), rig.streams[1], make("R2", rig.grid)[0])]
    hc, tc = rig.handle(4), rig.streams[3]
    for _, _, r in prod:
        run_alone(r, rig, monkeypatch)
    steps = [(r, r.outputs(0, rig.dev)) for _, _, r in prod]
    dest = [(r, r.outputs(1, rig.dev)) for _, _, r in prod]     # (the consumer's own packed bytes and offsets)

    def round_():
        for (h, ts, r), (_, outs), (_, mine) in zip(prod, steps, dest):
            issue(r, h, outs, ts, monkeypatch, post=False)
            ev = torch.cuda.Event()
            ev.record(ts)
            tc.wait_event(ev)
            hc.compact_ops_device(r.n, outs.ptr("ops"), r.dev["ops_off"].data_ptr(), outs.ptr("res", 4 * r.n), mine.ptr("packed"), r.n * r.slot,
                                  mine.ptr("packed_off"), tc.cuda_stream)
    torch.cuda.synchronize()
    round_()                                            # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    round_()                                            # rehearsal
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    gate_s = rig.gate_length(t_issue)
    _refill(steps + dest)
    gates = [rig.gate(ts, gate_s) for _, ts, _ in prod]
    round_()
    held = [not ev.query() for ev in gates]
    tc.synchronize()                                    # (the consumer's stream alone: its events cover the producers' steps)
    got = []
    for (r, outs), (_, mine) in zip(steps, dest):
        g = outs.host(("res", "ops"))
        g.update({k: v for k, v in mine.host(("packed", "packed_off")).items() if k in ("packed", "packed_off")})
        got.append((r, g))
    torch.cuda.synchronize()
    _report(record_property, test4_t_issue_s=t_issue, test4_gate_s=gate_s)
    assert all(held), "a gate (%.3f s) opened before the last call was issued (rehearsal: %.4f s): %s" % (gate_s, t_issue, held)
    for r, g in got:
        same(g, run_alone(r, rig, monkeypatch), r.sample(), only=("res", "ops", "packed", "packed_off"))


def _host_batches():
    return [("local", _ragged_pairs(500, 30, 150, 30, 150, 0xB0B)), ("global", _ragged_pairs(100, 100, 300, 100, 300, 0xB0C))]


def _check_host(res, mode, pairs):
    """a host-entry result against the oracle, every pair"""
    for k, (a, b) in enumerate(pairs):
        ref = O.align(O.MODE_NAMES[mode], a, b, *DEFAULT)
        assert ref["rc"] == 0
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]), res["ops"][k])
        assert got == (ref["score"], ref["end_i"], ref["end_j"], ref["state"], ref["ops"]), (mode, k)


@gpu
def test_host_entry_beside_queued_device_launches(rig, monkeypatch, record_property):
    """While a gated stream holds R1, R2 and R3 on handle A, the host entry of handle B (its own non-blocking stream, which is all it waits
    for) aligns two batches and returns while A's gate is still closed.

    Streams outnumber the card's hardware queues, and two streams that share one are served in issue order -- B's launches would then sit
    behind A's gate through no doing of the library.  So A's stream is chosen among the file's four by a probe beforehand: the first one
    behind whose (short) gate a small host-entry call returns.  The assertion proper is made once, on the full run."""
    import torch
    A_, B_ = rig.handle(1), rig.handle(2)
    steps = [(r, r.outputs(0, rig.dev)) for name in ("R1", "R2", "R3") for r in make(name, rig.grid)]
    for r, _ in steps:
        run_alone(r, rig, monkeypatch)
    batches = _host_batches()
    B_.set_scoring(*DEFAULT)
    B_.set_edit_traceback(False)
    for mode, pairs in batches:                         # warm-up of B: its staging and device buffers reach their size
        B_.align_batch(mode, pairs, render=False)
    torch.cuda.synchronize()
    probe, ts = [], rig.streams[0]
    for cand in rig.streams:
        ev = rig.gate(cand, 0.03)
        B_.align_batch("local", batches[0][1][:8], render=False)
        free = not ev.query()
        cand.synchronize()
        probe.append(free)
        if free:
            ts = cand
            break
    for r, outs in steps:                               # warm-up of A on that stream
        issue(r, A_, outs, ts, monkeypatch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()                            # rehearsal
    for r, outs in steps:
        issue(r, A_, outs, ts, monkeypatch)
    for mode, pairs in batches:
        B_.align_batch(mode, pairs, render=False)
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    gate_s = rig.gate_length(t_issue)
    _refill(steps)
    ev = rig.gate(ts, gate_s)
    for r, outs in steps:
        issue(r, A_, outs, ts, monkeypatch)
    res = [B_.align_batch(mode, pairs, render=False) for mode, pairs in batches]
    held = not ev.query()
    ts.synchronize()
    _report(record_property, test5_t_issue_s=t_issue, test5_gate_s=gate_s, test5_stream_probe=str(probe))
    assert held, "the host entry did not return while the other handle's gate (%.3f s) was closed (rehearsal: %.4f s; probe %s)" % (gate_s, t_issue, probe)
    for (mode, pairs), out in zip(batches, res):
        _check_host(out, mode, pairs)
    _compare(steps, rig, monkeypatch)
