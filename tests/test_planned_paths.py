"""Tracebacks on PLANNED paths: pairs built so that the optimal path holds a long vertical, horizontal or jump run, a staircase of
one-base gaps, a walk along a border, ties all over (low complexity), or an end and a HOME cell on chosen band and block edges.  The
other parity tests draw unrelated reads or reads with scattered edits, whose paths stay within a few columns of the diagonal -- where
every walker's prediction of the walk's way holds.  Here it fails, on purpose.

Three parts:
  1. generators (pure Python, seeded), each with a CONDITION on the oracle's ops that every generated pair meets;
  2. pattern_misses: a CPU model of which blocks a round of the two-pass tracebacks replays (CkPattern of at_sweep16.hip.h, restated),
     followed along the oracle's ops -- it says how often a pair's walk leaves its round's blocks sideways or outruns them
     (unmarked tests: no GPU);
  3. GPU parity: every pair of every case through every traceback engine that exists for its shape, every field against the oracle.

    python3 tests/test_planned_paths.py        # prints, per case, pairs and the model's miss counts (no GPU)
"""
import collections
import os
import random
import re
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                                 # (run as a script, or imported by the fuzzers)
import oracle as O

J0 = -10
LOW, UPP, JUMP = bytes([O.OP_LOW]), bytes([O.OP_UPP]), bytes([O.OP_JUMP])


# =============================================================================================== 1. generators

def _rnd(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _flank(rng, core, l2, left=None):
    """core inside l2 bases, random flanks (left flank of `left` bases, or drawn)"""
    pad = l2 - len(core)
    assert pad >= 0, (len(core), l2)
    if left is None:
        left = rng.randint(0, pad)
    return _rnd(rng, left) + core + _rnd(rng, pad - left)


def vertical(rng, mode, l1, l2, d, left=None, h=None):
    """s2 = s1 without d consecutive bases of its middle (global: l2 = l1 - d; else between random flanks): a LOW run of d"""
    s1 = _rnd(rng, l1)
    if h is None:
        h = (l1 - d) // 2 + rng.randint(-3, 3)
    core = s1[:h] + s1[h + d:]
    return s1, core if mode == "global" else _flank(rng, core, l2, left)


def horizontal(rng, mode, l1, l2, d, left=None, h=None):
    """s2 = s1 with d foreign bases in its middle (global: l2 = l1 + d; else between random flanks): an UPP (fit -s: JUMP) run of d"""
    s1 = _rnd(rng, l1)
    if h is None:
        h = l1 // 2 + rng.randint(-3, 3)
    core = s1[:h] + _rnd(rng, d) + s1[h:]
    return s1, core if mode == "global" else _flank(rng, core, l2, left)


def staircase(rng, mode, l1, l2):
    """s2 = s1 with a one-base deletion and a one-base insertion taking turns every 6 bases (l2 = l1 or l1 +- 1 before the flanks)"""
    s1 = _rnd(rng, l1)
    t = []
    for k in range(0, l1, 6):
        seg = s1[k:k + 6]
        if len(seg) == 6:
            seg = seg[:3] + seg[4:] if (k // 6) % 2 == 0 else seg[:3] + rng.choice("ACGT") + seg[3:]
        t.append(seg)
    core = "".join(t)
    return s1, core if l2 is None else _flank(rng, core, l2)


def staircase_len(l1):
    """the length of staircase()'s second sequence before any flank"""
    full = l1 // 6
    return l1 - (full + 1) // 2 + full // 2


def corner(l1, l2, K, CB, k, rng):
    """local: s1 = A.. + core + A.., s2 = C.. + core + C.., core over GT -- the alignment is the core, from (x + 1, y + 1) to
    (x + c, y + c).  Pair k puts the first and the last row on, one before and one after a band edge (a multiple of K rows), and the
    last (even k) or the first (odd k) cell's step t = column - 1 + band on, one before or one after a block edge (a multiple of CB)."""
    nb = l1 // K
    a = 1 + k % max(1, nb - 2)
    b = min(nb, a + 1 + (k // 3) % max(1, nb - a))
    first = a * K + (-1, 0, 1, 2)[k % 4]                     # row of the first cell: the band's last two rows, the next one's first two
    last = min(l1, b * K + (0, 1, -1)[(k // 4) % 3])         # row of the last cell
    c = last - first + 1
    x = first - 1
    want = (CB - 1, 0, 1)[(k // 12) % 3]                     # t % CB of the chosen cell
    if k % 2 == 0:
        base = c - 1 + (last - 1) // K                       # t of the last cell = y + base
    else:
        base = (first - 1) // K                              # t of the first cell = y + base
    y = (want - base) % CB + CB * ((k // 36) % max(1, (l2 - c - CB) // CB))
    assert 0 < x and 0 < c and x + c <= l1 and 0 <= y and y + c <= l2, (l1, l2, K, CB, k, x, y, c)
    core = _rnd(rng, c, "GT")
    return ("A" * x + core + "A" * (l1 - x - c), "C" * y + core + "C" * (l2 - y - c)), dict(x=x, y=y, c=c)


def low_complexity(rng, l1, l2, k):
    """homopolymers with a foreign base now and then, dinucleotide repeats with a one-base slip (tests/test_local_pointer_cell.py)"""
    from test_local_pointer_cell import _pair
    return _pair(rng, l1, l2, 8 * (k // 2) + 1 + k % 2)


def max_run(ops, op):
    return max((len(m) for m in re.findall(re.escape(op) + b"+", ops)), default=0)


def gap_runs(ops):
    return len(re.findall(b"\x01+|\x02+", ops))


def planned_pair(rng, mode, l1, l2, alpha="ACGT"):
    """for the fuzzers: a pair of l1 x l2 from a draw among vertical, horizontal and staircase, the run's length among the edges of
    the walkers' looks and the rounds' patterns; cut or filled to l2 bases"""
    kind = rng.choice(["vertical", "horizontal", "staircase"])
    if kind == "vertical":
        d = rng.choice([d for d in (4, 5, 15, 16, 17, 20, 33, 40, 100, 400) if d < l1 // 2])
        s1, core = vertical(rng, "global", l1, None, d)
    elif kind == "horizontal":
        d = rng.choice([d for d in (15, 16, 17, 31, 32, 33, 127, 128, 129, 200, 400) if d <= max(15, l2 - l1)])
        s1, core = horizontal(rng, "global", l1, None, d)
    else:
        s1, core = staircase(rng, "global", l1, None)
    if alpha != "ACGT":                                      # (byte alphabets: a foreign letter in each read)
        q = rng.randrange(len(s1))
        s1 = s1[:q] + rng.choice(alpha) + s1[q + 1:]
    pre = _rnd(rng, rng.randint(0, max(0, l2 - len(core))), alpha)
    return s1, (pre + core + _rnd(rng, l2, alpha))[:l2]


# ----------------------------------------------------------------------------------------------- the cases

SG1, SG2 = (1, -1, -4, -1), (2, -2, -5, -2)        # global
SF1, SF2 = (1, -3, -4, -1), (2, -4, -5, -1)        # fit
SL2, SL0 = (2, -2, -5, -1), (2, -2, -5, 0)         # local (SL0: horizontal runs of any length cost one opening)
SJ2, SJ1 = (2, -2, -5, -1, -10), (1, -1, -4, -1, -6)   # fit -s
# ... for 620 x 1 060: with e = -1 the scores of that shape leave the x16 range, and fit -s has two-pass kernels for x16 only
SJ0 = (1, -1, -8, 0, -6)
ST = [(2, -3, -1, -1), (3, -3, 0, -1), (1, -1, -1, -1)]  # staircases

E8 = ("int32", "onepass", "onepass16", "rounds", "walk", "teams", "default")   # 8 lanes x 19 rows: reads of 129 .. 152 bases
E64 = ("int32", "onepass", "rounds", "walk", "teams", "default")               # 64 lanes x 16 rows: reads of 609 .. 1 024 bases
E1 = ("int32", "onepass")                                                        # every other group width: no two-pass kernels

ENGINES = {
    # name: (environment, what last_config must hold, what it must not hold)
    "int32": ({"AT_NO_PACKED": "1"}, ("int32",), ("packed16",)),
    "onepass": ({"AT_TWO_PASS": "0"}, ("packed16",), ("two-pass",)),
    "onepass16": ({"AT_TWO_PASS": "0", "AT_GROUP": "16"}, ("packed16", "4x16-lane"), ("two-pass",)),
    "rounds": ({"AT_TWO_PASS": "2", "AT_TP_SPLIT": "0"}, ("two-pass",), ("walk kernel",)),
    "walk": ({"AT_TWO_PASS": "2", "AT_TP_SPLIT": "1", "AT_WALK_TEAMS": "0"}, ("walk kernel",), ("teams",)),
    "teams": ({"AT_TWO_PASS": "2", "AT_TP_SPLIT": "1", "AT_WALK_TEAMS": "1"}, ("walk kernel", "teams"), ()),
    "default": ({}, (), ()),
}
GROUPS = {4: "16x4-lane groups", 8: "8x8-lane groups", 16: "4x16-lane groups", 32: "2x32-lane groups", 64: "1x64-lane groups"}
KNOBS_CLEARED = ("AT_TWO_PASS", "AT_TP_SPLIT", "AT_GROUP", "AT_STORE", "AT_NO_PACKED", "AT_WS_CAP_MB", "AT_WALK_TEAMS", "AT_CK_PIECE_PAIRS",
                 "AT_TAIL_SPLIT", "AT_ROWS_PER_LANE", "AT_CK_CAP_MB")


class Case:
    def __init__(self, kind, mode, sc, l1, l2, d=0, engines=E8, n=None, with_n=False, cfg=(), h0=None):
        self.kind, self.mode, self.l1, self.l2, self.d, self.engines, self.with_n, self.cfg, self.h0 = kind, mode, l1, l2, d, engines, with_n, cfg, h0
        self.sc = tuple(sc) + ((J0,) if len(sc) == 4 else ())
        self.uj = kind == "jump"
        self.n = n if n is not None else 129 if l1 <= 152 else 33
        self.grid = (8, 19, 16) if 129 <= l1 <= 152 else (64, 16, 32) if 609 <= l1 <= 1024 else None   # G, K, CB of the two-pass kernels
        # What the model must show for every pair: a vertical run that leaves the round's blocks sideways, a horizontal or jump run that
        # outruns the horizontal pattern.  On the 8-lane groups that takes a chosen placement (place), as the 2 049 columns do (h0)
        self.tune = None
        if self.grid and kind == "vertical" and d >= (100 if self.grid[0] == 64 else 17):
            self.tune = "sideways"
        if self.grid and kind in ("horizontal", "jump") and d >= (2049 if self.grid[0] == 64 else 129):
            self.tune = "outrun"
        self._place, self._built = None, {}
        self.id = "%s%s-%s-%dx%d%s-m%d%d%d%d%s" % (kind, "-d%d" % d if d else "", mode, l1, l2, "-N" if with_n else "", self.sc[0], -self.sc[1], -self.sc[2],
                                                  -self.sc[3], "j%d" % -self.sc[4] if self.uj else "")

    @property
    def place(self):
        """(h, left): the row of s1 behind which the run sits and the left flank of s2, where they are the batch's and not each pair's.
        A jump's intron sits at the same columns in every pair (the site list is the batch's), in the middle of the read behind a
        flank of 20 bases.  Where the model must show a miss for every pair, the spot nearest to the middle at which it does for a
        sample -- an outrun needs the run's first cell to be the first cell of a round.  Else (None, None): drawn pair by pair."""
        if self._place is None:
            mid = (self.l1 - self.d) // 2 if self.kind == "vertical" else self.l1 // 2
            if self.h0 is not None:
                spots = [(self.h0, 0)]
            elif self.tune and self.grid[0] == 8:
                pad = self.l2 - (self.l1 - self.d if self.kind == "vertical" else self.l1 + self.d)
                flanks = [0] if self.mode == "global" else range(min(20, max(0, pad - 15)), min(pad, 35) + 1)
                top = min(mid + 46, self.l1 - 12 - (self.d if self.kind == "vertical" else 0))
                spots = sorted(((h, f) for h in range(max(12, mid - 45), top) for f in flanks), key=lambda v: abs(v[0] - mid) + v[1])
            else:
                spots = [(mid, 20)] if self.uj else [(None, None)]
            for self._place in spots:
                rng = random.Random(zlib.crc32(self.id.encode()) + 64 * (self._place[0] or 0) + (self._place[1] or 0))
                if len(spots) == 1 or sum(self.planned(self.draw(rng, k)) for k in range(4)) >= 2:   # (build redraws a pair whose run a tie slides away)
                    break
            else:
                raise AssertionError((self.id, "no placement shows the planned miss"))
        return self._place

    @property
    def sites(self):
        """jump: the columns before and behind the intron"""
        return [self.place[1] + self.place[0] - 1, self.place[1] + self.place[0] + self.d + 1] if self.uj else []

    def draw(self, rng, k):
        """pair k and what the oracle must show for it"""
        exp = {}
        h, left = self.place if self.kind in ("vertical", "horizontal", "jump") else (None, None)
        if self.kind == "vertical":
            p = vertical(rng, self.mode, self.l1, self.l2, self.d, left, h)
        elif self.kind in ("horizontal", "jump"):
            p = horizontal(rng, self.mode, self.l1, self.l2, self.d, left, h)
        elif self.kind == "staircase":
            p = staircase(rng, self.mode, self.l1, None if self.mode == "global" else self.l2)
        elif self.kind == "border":
            p = _rnd(rng, self.l1), _rnd(rng, self.l2)
        elif self.kind == "lowcx":
            p = low_complexity(rng, self.l1, self.l2, k)
        else:
            p, exp = corner(self.l1, self.l2, self.grid[1], self.grid[2], k, rng)
        assert (len(p[0]), len(p[1])) == (self.l1, self.l2), (self.id, k, len(p[0]), len(p[1]))
        return p, exp

    def planned(self, drawn):
        """does the oracle's walk of this pair show the case's condition and what the model must show?"""
        p, exp = drawn
        r = _oracle(self, [p])[0]
        if r["rc"] != 0 or self.condition(r, exp) is not None:
            return False
        m = pattern_misses(r["ops"], r["end_i"], r["end_j"], r["state"], *self.grid)
        return (m.sideways if self.tune == "sideways" else m.outrun) >= 1

    def build(self, n=None):
        """the first n pairs of the case (a prefix of the whole batch) and, per pair, what the oracle must show"""
        n = self.n if n is None else n
        if n in self._built:
            return self._built[n]
        rng = random.Random(zlib.crc32(self.id.encode()))
        pairs, expect = [], []
        for k in range(n):
            p, exp = self.draw(rng, k)
            if self.tune and self.place[0] is not None:   # (a tie may slide the run off its place: the bases are drawn again)
                for _ in range(400):
                    if self.planned((p, exp)):
                        break
                    p, exp = self.draw(rng, k)
                else:
                    raise AssertionError((self.id, k, "no placement shows the planned miss"))
            if self.with_n and k == n // 2:          # one N in one read: the whole batch travels as byte words
                q = self.l1 // 3
                p = (p[0][:q] + "N" + p[0][q + 1:], p[1])
            pairs.append(p)
            expect.append(exp)
        self._built[n] = pairs, expect
        return pairs, expect

    def condition(self, r, exp):
        """None if the oracle's result r shows what the case plans, else what it shows instead"""
        ops = r["ops"]
        if self.kind == "vertical":
            return None if max_run(ops, LOW) >= self.d else ("LOW run", max_run(ops, LOW))
        if self.kind == "horizontal":
            return None if max_run(ops, UPP) >= self.d else ("UPP run", max_run(ops, UPP))
        if self.kind == "jump":
            return None if max_run(ops, JUMP) >= self.d - 2 else ("JUMP run", max_run(ops, JUMP))
        if self.kind == "staircase":
            return None if 8 * gap_runs(ops) >= self.l1 else ("gap runs", gap_runs(ops))
        if self.kind == "border":
            op = UPP if self.l2 > self.l1 else LOW
            return None if max_run(ops, op) >= 30 else ("border run", max_run(ops, op))
        if self.kind == "corner":
            # the walk emits the op of the cell whose pointer says HOME: the core's c cells and the A / C cell before it, then HOME
            # (y = 0: the core starts in column 1 and the walk ends at the border instead)
            n = exp["c"] + (1 if exp["y"] > 0 else 0)
            got = (r["end_i"], r["end_j"], len(ops), r["state"], ops.count(b"\x00"))
            want = (exp["x"] + exp["c"], exp["y"] + exp["c"], n, 2, n)
            return None if got == want else (got, want)
        return None


def _cases():
    out = []
    # ---- reads of 150 bases: 8 lanes x 19 rows (K + 1 = 20; 17 rows: a band and one; the rounds' margin is 3 steps)
    for d in (4, 5, 17, 20, 40):
        out.append(Case("vertical", "global", SG1 if d in (4, 17, 40) else SG2, 150, 150 - d, d))
        out.append(Case("vertical", "fit", SF2 if d in (4, 17, 40) else SF1, 150, 230, d))
        out.append(Case("vertical", "local", SL2, 150, 150, d))
    for d in (15, 16, 17, 127, 128, 129, 200):
        out.append(Case("horizontal", "global", SG1, 150, 150 + d, d))
        out.append(Case("horizontal", "local", SL0, 150, 150 + d + 20, d))
        if d != 200:
            out.append(Case("horizontal", "fit", SF2, 150, max(230, 150 + d + 20), d))
    for d in (15, 16, 17, 31, 32, 33, 127, 128, 129, 257):
        out.append(Case("jump", "fit", SJ2, 150, max(230, 150 + d + 40), d))
    out.append(Case("staircase", "global", ST[0], 150, staircase_len(150)))
    out.append(Case("staircase", "local", ST[1], 150, 160))
    out.append(Case("staircase", "global", ST[2], 150, staircase_len(150)))
    out.append(Case("border", "global", SG1, 150, 1))
    out.append(Case("border", "global", SG1, 152, 2))
    out.append(Case("border", "global", SG1, 150, 1200))
    for mode, sc in (("local", ST[2]), ("global", ST[2]), ("fit", SF1)):
        out.append(Case("lowcx", mode, sc, 150, 500))
    out.append(Case("corner", "local", SG2, 150, 150))
    out.append(Case("corner", "local", ST[2], 152, 230))
    out.append(Case("vertical", "global", SG1, 150, 133, 17, with_n=True, cfg=("bits=8",)))
    # ---- reads of 133 bases: seven lanes of the eight filled exactly
    out.append(Case("vertical", "fit", SF1, 133, 200, 20))
    out.append(Case("horizontal", "global", SG1, 133, 133 + 129, 129))
    out.append(Case("jump", "fit", SJ2, 133, 230, 16))
    out.append(Case("staircase", "local", ST[1], 133, 140))
    # ---- reads of 620 and 1 000 / 1 024 bases: 64 lanes x 16 rows (the rounds' margin is 40 steps, 3 blocks of 32 per band)
    for d in (17, 33, 100, 400):
        out.append(Case("vertical", "global", SG1 if d in (17, 100) else SG2, 1000, 1000 - d, d, E64, cfg=() if d in (17, 100) else ("packed16 x4 ",)))
        out.append(Case("vertical", "fit", SF1 if d in (33, 400) else SF2, 1000, 1024, d, E64))
        out.append(Case("vertical", "local", SL2, 1000, 1000, d, E64))
    out.append(Case("vertical", "local", SG1, 620, 620, 33, E64, cfg=("packed16 x16 ",)))
    for d in (31, 32, 33, 100, 400):
        out.append(Case("horizontal", "global", SG1, 1000, 1000 + d, d, E64))
        out.append(Case("horizontal", "local", SL0, 1000, 1000 + d + 24, d, E64))
    for d in (2047, 2049):   # one column under and over the 64-lane horizontal pattern (64 blocks of 32 columns)
        out.append(Case("horizontal", "global", SG1, 620, 620 + d, d, E64, n=12, h0=288 if d == 2049 else None))
    for d in (16, 33, 400):
        out.append(Case("jump", "fit", SJ1 if d < 400 else SJ0, 620, 620 + d + 40, d, E64, cfg=("packed16 x16 ",)))
    out.append(Case("staircase", "global", ST[0], 1000, staircase_len(1000), 0, E64))
    out.append(Case("staircase", "local", ST[2], 1000, 1024, 0, E64, cfg=("packed16 x16 ",)))
    out.append(Case("staircase", "global", ST[1], 620, staircase_len(620), 0, E64))
    out.append(Case("border", "global", SG1, 1024, 40, 0, E64))
    out.append(Case("border", "global", SG1, 700, 3, 0, E64))
    for mode, sc in (("local", SG2), ("global", SG2), ("fit", SF1)):
        out.append(Case("lowcx", mode, sc, 1000, 1024, 0, E64))
    out.append(Case("corner", "local", SG2, 1000, 1000, 0, E64))
    out.append(Case("corner", "local", ST[2], 1024, 1100, 0, E64))
    out.append(Case("horizontal", "global", SG1, 1000, 1033, 33, E64, with_n=True, cfg=("bits=8",)))
    # ---- the other group widths: one-pass and int32 engines only
    out.append(Case("border", "global", SG1, 40, 1024, 0, E1))
    for l1, dv, dh in ((60, 17, 17), (300, 33, 33), (500, 100, 129), (2000, 400, 100)):
        # 60: 4-lane groups; 300: 16 x 19; 500: 32 x 16; 2 000: the 64-lane group in strips of 256 rows, rows 800 .. 1 200 cross a strip's edge
        out.append(Case("vertical", "global", SG1, l1, l1 - dv, dv, E1))
        out.append(Case("horizontal", "global", SG1, l1, l1 + dh, dh, E1))
        out.append(Case("staircase", "global", ST[2], l1, staircase_len(l1), 0, E1))
    out.append(Case("vertical", "global", SG1, 300, 283, 17, E1, with_n=True, cfg=("bits=8",)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}

_CACHE = {}


def _oracle(case, pairs):
    """the oracle's result for every distinct pair, once per scoring, site list and pair"""
    memo = _CACHE.setdefault((case.mode, case.sc, tuple(case.sites)), {})
    todo = [p for p in dict.fromkeys(pairs) if p not in memo]
    if todo:
        O.align(O.LOCAL, "A", "AA")                  # (loads the library before the threads start)
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            res = list(ex.map(lambda p: O.align(O.MODE_NAMES[case.mode], p[0], p[1], *case.sc, case.uj, case.sites), todo))
        memo.update(zip(todo, res))
    return [memo[p] for p in pairs]


# =============================================================================================== 2. the model of a round's blocks

Misses = collections.namedtuple("Misses", "sideways overflow outrun")


def pattern_misses(ops, end_i, end_j, state, G, K, CB):
    """The oracle's walk (ops from the end cell, its start state) followed through the rounds of a two-pass traceback on groups of G
    lanes x K rows with blocks of CB steps: Misses(sideways, overflow, outrun) -- how often the walk steps into a block that has no
    slot in the current round while bands remain (sideways), and how often because the round's bands or its G horizontal blocks ran
    out (overflow; outrun counts those of them where a horizontal round's G blocks of the anchor's band ran out under a walk that
    still runs left).  Every miss starts the next round at that cell, as in the kernels.

    A restatement of CkPattern, aligntools/c_amd/csrc/at_sweep16.hip.h: the constants :496-503, set :505-510, ctop :511, band
    :513-523, slot :541-557; its use by the walks :1643 / :1687-1690 (rounds) and at_walk16.hip.h :606 / :624-626 (teams).  A change
    there needs one here.

    G is the number of blocks a round replays per alignment: the group's lanes for the rounds inside the sweep's kernel (8 x 19 with
    CB = 16, 64 x 16 with CB = 32: GRID), the team's lanes for the walk kernel's teams (2 and 4: TEAM_GRID; CkPattern<NT, K, CB>, the
    narrow form on both group widths).  The walk kernel with one walker per half-lane replays the one block its walker stands in."""
    LCB = CB.bit_length() - 1
    FIXED, W = G == 64, 3                                    # :500-501 (AT_CK_W64)
    NB = G // W
    MH = min(max((W * CB - K) // 2, 0), CB)                  # :502
    MU = ML = 3                                              # :503
    pat = {}

    def set_(ci, cj, hz):                                    # :505-510
        b = (ci - 1) // K
        rho, T0 = (ci - 1) - b * K, cj - 1 + b
        pat.update(b=b, c0=T0 >> LCB, thi1=T0 - rho - 2, horiz=hz)

    def ctop(dr):                                            # :511 (>> floors, as the arithmetic shift does)
        return pat["c0"] if dr == 0 else (pat["thi1"] - (dr - 1) * (K + 1) + MH) >> LCB

    def band(dr):                                            # :513-523 -> (chi, n)
        if FIXED:
            return ctop(dr), W
        thi = pat["thi1"] - (dr - 1) * (K + 1)
        tlo = pat["thi1"] + 2 if dr == 0 else thi - (K - 1)
        chi = pat["c0"] if dr == 0 else (thi + MU) >> LCB
        clo = max((tlo - ML) >> LCB, 0)
        return chi, max(chi - clo + 1, 0)

    SIDE, BANDS, BLOCKS = "sideways", "bands ran out", "horizontal blocks ran out"

    def slot(bl, c):                                         # :541-557 -> (slot, None) or (-1, why)
        dr = pat["b"] - bl
        if pat["horiz"]:
            w = pat["c0"] - c
            return (w, None) if dr == 0 and 0 <= w < G else (-1, BLOCKS if dr == 0 and w >= G else BANDS)   # (one band: any other is out)
        if FIXED:
            if dr < 0 or dr >= NB:
                return -1, BANDS
            w = ctop(dr) - c
            return (dr * W + w, None) if 0 <= w < W else (-1, SIDE)
        if dr < 0:
            return -1, BANDS
        s0 = 0
        for x in range(dr):
            s0 += band(x)[1]
            if s0 >= G:
                return -1, BANDS
        chi, n = band(dr)
        w = chi - c
        if 0 <= w < n:
            return (s0 + w, None) if s0 + w < G else (-1, BANDS)
        return -1, SIDE

    ci, cj = end_i, end_j
    count = {SIDE: 0, BANDS: 0, BLOCKS: 0}
    first = True
    for op in ops:
        if ci <= 0 or cj <= 0:                               # a border: the rounds are over (global: the padding loops)
            break
        hz = op in (O.OP_UPP, O.OP_JUMP)                     # the state the walk is in at this cell: :1643
        if first:
            assert op == {1: O.OP_LOW, 2: O.OP_MID, 3: O.OP_UPP}[state], (op, state)
            set_(ci, cj, hz)
            first = False
        bl = (ci - 1) // K                                   # :1687-1689
        q, why = slot(bl, ((cj - 1) + bl) >> LCB)
        if q < 0:
            count[why] += 1
            set_(ci, cj, hz)
            assert slot(bl, ((cj - 1) + bl) >> LCB)[0] == 0  # (the anchor's own block is slot 0 of its round)
        ci -= op in (O.OP_MID, O.OP_LOW)
        cj -= op in (O.OP_MID, O.OP_UPP, O.OP_JUMP)
    return Misses(count[SIDE], count[BANDS] + count[BLOCKS], count[BLOCKS])


TEAM_GRID = {8: (2, 19, 16), 64: (4, 16, 32)}     # AT_WALK_TEAM8, AT_WALK_TEAM (at_k16_walk8.hip, at_k16_walk64.hip): lanes of a team, K, CB


def _misses(case, refs, teams=False):
    grid = TEAM_GRID[case.grid[0]] if teams else case.grid
    return [pattern_misses(r["ops"], r["end_i"], r["end_j"], r["state"], *grid) for r in refs]


def scattered_control(l1, l2, n):
    """related pairs as tests/test_gpu_parity.py::test_two_pass_tracebacks draws them: 1 + l1 // 15 scattered edits"""
    rng = random.Random(l1 * 7919 + l2)
    out = []
    for _ in range(n):
        a = _rnd(rng, l1)
        t = list(a)
        for _ in range(1 + l1 // 15):
            q = rng.randrange(len(t))
            r = rng.random()
            if r < 0.5:
                t[q] = rng.choice("ACGT")
            elif r < 0.75 and len(t) > 1:
                del t[q]
            else:
                t.insert(q, rng.choice("ACGT"))
        out.append((a, (_rnd(rng, rng.randint(0, max(0, l2 - l1))) + "".join(t) + _rnd(rng, l2))[:l2]))
    return out


CPU_PAIRS = 8


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_condition_holds_for_every_pair(case):
    """the plan, checked on the oracle: every pair's ops show the run, the staircase, the border walk or the anchors the case is for"""
    pairs, expect = case.build(CPU_PAIRS)
    refs = _oracle(case, pairs)
    assert all(r["rc"] == 0 for r in refs), case.id
    bad = [(k, case.condition(r, e)) for k, (r, e) in enumerate(zip(refs, expect)) if case.condition(r, e) is not None]
    assert not bad, (case.id, bad)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "vertical" and c.grid and c.d >= (100 if c.grid[0] == 64 else 17)], ids=lambda c: c.id)
def test_vertical_runs_leave_the_round_sideways(case):
    """a LOW run longer than the pattern's margin (40 steps on 64 x 16, 3 on 8 x 19) climbs out of the blocks along the diagonal ray"""
    refs = _oracle(case, case.build(CPU_PAIRS)[0])
    assert min(m.sideways for m in _misses(case, refs)) >= 1, (case.id, _misses(case, refs))


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("horizontal", "jump") and c.grid and c.d >= (2049 if c.grid[0] == 64 else 129)], ids=lambda c: c.id)
def test_horizontal_runs_outrun_the_round(case):
    """an UPP or JUMP run of more than G blocks' columns (128 on 8 lanes, 2 048 on 64) outruns the horizontal pattern"""
    refs = _oracle(case, case.build(CPU_PAIRS)[0])
    assert min(m.outrun for m in _misses(case, refs)) >= 1, (case.id, _misses(case, refs))


def test_one_column_under_the_horizontal_pattern_stays_inside():
    """A run that the walk enters inside a round leaves that round's blocks at a block's edge, where the next, horizontal round holds
    64 x 32 = 2 048 columns: the 2 047 that are left at the most fit.  (The 2 049 case puts its run in row 288, the first row the
    walk from row 620 meets when its round's 21 bands are spent: the round that starts on the run's first cell holds 2 017 .. 2 048.)"""
    case = BY_ID["horizontal-d2047-global-620x2667-m1141"]
    refs = _oracle(case, case.build(CPU_PAIRS)[0])
    assert max(m.outrun for m in _misses(case, refs)) == 0, _misses(case, refs)


def test_scattered_edits_stay_inside_the_pattern():
    """the control: related pairs of the existing two-pass tests never leave a round of the 64-lane group sideways -- for the rounds
    inside the sweep's kernel what this module plants is new to the suite"""
    for mode, l1, l2, sc in (("global", 1024, 1024, SG1), ("local", 1000, 1024, SG2), ("fit", 700, 1024, SG1)):
        case = Case("control", mode, sc, l1, l2, 0, E64)
        refs = _oracle(case, scattered_control(l1, l2, CPU_PAIRS))
        assert all(len(r["ops"]) > l1 // 2 for r in refs), (mode, [len(r["ops"]) for r in refs])
        assert max(m.sideways for m in _misses(case, refs)) == 0, (mode, l1, l2, _misses(case, refs))
        # (a team of 4 lanes spends its 4 blocks in two or three bands, 17 .. 27 times per pair, and a block is 32 steps wide against
        # drifts of a few columns: 1 sideways miss in these 24 pairs)
        assert sum(m.sideways for m in _misses(case, refs, teams=True)) <= 1 * len(refs), (mode, l1, l2, _misses(case, refs, teams=True))


def test_model_on_hand_made_walks():
    """pattern_misses itself: a diagonal walk never misses sideways and runs out of bands every NB = 21 bands (64 x 16) or when its
    8 slots are spent (8 x 19); a straight climb leaves the 8 x 19 pattern in the band above the anchor's"""
    diag = bytes([O.OP_MID]) * 1000
    assert pattern_misses(diag, 1000, 1000, 2, 64, 16, 32) == (0, 2, 0)      # (from band 62: the rounds start in bands 62, 41 and 20)
    m = pattern_misses(diag[:150], 150, 150, 2, 8, 19, 16)
    assert m.sideways == 0 and 1 <= m.overflow <= 8 and m.outrun == 0, m
    m = pattern_misses(LOW * 60, 100, 50, 1, 8, 19, 16)                      # (band 4 still holds its step; bands 3 and 2 do not)
    assert m.sideways >= 2 and m.overflow == 0, m
    assert pattern_misses(UPP * 129, 100, 140, 3, 8, 19, 16) == (0, 1, 1)    # (t = 144: blocks 9 .. 2, columns 140 .. 28; 12 are left)
    assert pattern_misses(UPP * 113, 100, 140, 3, 8, 19, 16) == (0, 0, 0)


# =============================================================================================== 3. GPU parity

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


def run_engine(al, case, engine, setenv, delenv):
    """the case's whole batch through one engine, every pair and every field against the oracle.  Returns last_config."""
    env, must, must_not = ENGINES[engine]
    for name in KNOBS_CLEARED:
        delenv(name)
    setenv("AT_HOST_CHUNKS", "1")      # (a chunk on a helper handle would keep its own last_config)
    setenv("AT_PACKED_MIN_ROUNDS", "0")
    for name, value in env.items():
        setenv(name, value)
    pairs, expect = case.build()
    refs = _oracle(case, pairs)
    bad = [(k, case.condition(r, e)) for k, (r, e) in enumerate(zip(refs, expect)) if r["rc"] != 0 or case.condition(r, e) is not None]
    assert not bad, (case.id, bad)
    al.set_scoring(*case.sc, case.uj, list(case.sites))
    res = al.align_batch(case.mode, pairs, traceback=True, render=False)
    cfg = al.last_config
    where = (case.id, engine, cfg)
    if engine in ("onepass", "rounds", "walk", "teams"):     # the class the case is for: its group width, rows per lane of the two-pass kernels
        width = GROUPS[case.grid[0] if case.grid else min(g for top, g in ((76, 4), (304, 16), (608, 32), (1 << 30, 64)) if case.l1 <= top)]
        must += (width,) + (("rows/lane=%d " % case.grid[1],) if engine != "onepass" else ())
    for text in must + (case.cfg if engine not in ("int32", "default") else ()):
        assert text in cfg, (text, where)
    for text in must_not:
        assert text not in cfg, (text, where)
    for k, r in enumerate(refs):
        got = (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k]), int(res["nops"][k]))
        assert got == (r["score"], r["end_i"], r["end_j"], r["state"], len(r["ops"])), (k, got, where)
        assert res["ops"][k] == r["ops"], (k, where)
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize("case,engine", [(c, e) for c in CASES for e in c.engines], ids=lambda v: v.id if isinstance(v, Case) else v)
def test_every_engine_matches_the_oracle(al, monkeypatch, case, engine):
    run_engine(al, case, engine, monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False))


if __name__ == "__main__":
    # per case: pairs, and the model's (sideways, overflow) misses, the minimum and the maximum over the whole batch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for c in CASES:
        pairs, expect = c.build()
        refs = _oracle(c, pairs)
        bad = [k for k, (r, e) in enumerate(zip(refs, expect)) if r["rc"] != 0 or c.condition(r, e) is not None]
        line = "%-46s pairs %3d  condition fails %d" % (c.id, len(pairs), len(bad))
        for teams in (False, True) if c.grid else ():
            m = _misses(c, refs, teams)
            line += "  %dx%d" % (TEAM_GRID[c.grid[0]] if teams else c.grid)[:2]
            line += "".join("  %s %d..%d" % (f, min(getattr(x, f) for x in m), max(getattr(x, f) for x in m)) for f in Misses._fields)
        print(line + (" " + str([(k, c.condition(refs[k], expect[k])) for k in bad[:3]]) if bad else ""), flush=True)
