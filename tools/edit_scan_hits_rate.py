#!/usr/bin/env python3
"""edit_scan_hits_rate.py -- what at_scan_hits (every occurrence of a read under a distance cutoff) costs beside at_scan
with the same cutoff, on one GPU; one JSON line per read set, appended to profiles/r12/edit_scan_hits_rate.jsonl.

    python3 tools/edit_scan_hits_rate.py [--turns 3] [--seconds 1.0] [--out FILE]

Read sets: the sizes of tools/edit_scan_rate.py, 4 096 reads of 150 bases and 1 024 reads of 1 000 bases, in one seeded target of
300 000 bases.  The target is three copies of one random 100 000-base segment, the second and third with 2 % substitutions of their
own; a read is a window of the first copy with 4 % substitutions, so every read lies at three loci.  max_dist = l1 / 8, min_sep = the
read's length, forward strand.  Four forms, each warmed up once, then taking turns; within a turn a form is repeated until `seconds`
have passed, and a turn's figure is the median:
    a   the baseline: the sweep phase of at_scan with cutoff = max_dist (key slots, at_scan<W, false>, unpack, merge), the device time
        at_last_config reports as sweep=..ms -- the kernel of DESIGN.md 3.12, unchanged
    b   the hits sweep, at_scan<W, true> alone: sweep=..ms of at_scan_hits' at_last_config
    c   sort, marking, prefix sums and compaction of the candidates: select=..ms of the same text
    d   at_scan_hits end to end from host memory, without and with CIGARs (wall clock)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aligntools.c_amd as A  # noqa: E402

SEG = 100000
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _noisy(rng, codes, rate):
    out = codes.copy()
    sub = rng.random(len(out)) < rate
    out[sub] = (out[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
    return out


def make_set(seed, nq, l1):
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 4, size=SEG)
    target = np.concatenate([seg, _noisy(rng, seg, 0.02), _noisy(rng, seg, 0.02)])
    at = rng.integers(0, SEG - l1, size=nq)
    queries = [bytes(ACGT[_noisy(rng, seg[a:a + l1], 0.04)]) for a in at]
    return queries, bytes(ACGT[target])


def until(seconds, fn):
    out, t0 = [], time.perf_counter()
    while not out or time.perf_counter() - t0 < seconds:
        out.append(fn())
    return out


def _ms(cfg, name):
    return float(cfg.rsplit(name + "=", 1)[1].split("ms")[0])


def measure(seed, nq, l1, turns, seconds):
    queries, target = make_set(seed, nq, l1)
    max_dist = l1 // 8
    al = A.Aligner(0)
    al.set_scoring(1, 1, -5, -1, -10)
    last = {}

    def form_a():
        last["a"] = al.scan(queries, [target], cutoff=max_dist)
        last["a_cfg"] = al.last_config
        return _ms(al.last_config, "sweep")

    def hits_call(cigar):
        t0 = time.perf_counter()
        last["d"] = al.scan_hits(queries, [target], max_dist, cigar=cigar)
        wall = (time.perf_counter() - t0) * 1e3
        cfg = al.last_config.split("; windows:")[0]
        last["b_cfg"] = al.last_config
        return _ms(cfg, "sweep"), _ms(cfg, "select"), wall

    form_a(); hits_call(False); hits_call(True)                          # warm-up of each form
    ms = {k: [] for k in ("a", "b", "c", "d", "d_cigar")}
    for _ in range(turns):
        ms["a"].append(float(np.median(until(seconds, form_a))))
        runs = until(seconds, lambda: hits_call(False))
        ms["b"].append(float(np.median([r[0] for r in runs])))
        ms["c"].append(float(np.median([r[1] for r in runs])))
        ms["d"].append(float(np.median([r[2] for r in runs])))
        ms["d_cigar"].append(float(np.median([r[2] for r in until(seconds, lambda: hits_call(True))])))
    cfg = last["b_cfg"]
    counts = {k: int(cfg.split(k + "=")[1].split()[0].rstrip(";")) for k in ("candidates", "kept", "resweeps")}
    per_read = np.diff(last["d"]["hit_off"])
    # the best hit of every read that at_scan finds under the cutoff is this entry's first
    a = last["a"]
    found = a["nhits"] > 0
    first = last["d"]["hit_off"][:-1][found]
    assert (per_read[found] > 0).all() and np.array_equal(last["d"]["score"][first], a["score"][found, 0]) \
        and np.array_equal(last["d"]["end_j"][first], a["end_j"][found, 0]), "at_scan's hit is not the first hit"
    al.close()
    rec = dict(what="scan-hits: %d reads of %d at three loci each in one target of %d, forward strand, max_dist=%d, min_sep=read" % (nq, l1, 3 * SEG, max_dist),
               reads=nq, l1=l1, l2=3 * SEG, max_dist=max_dist, turns=turns, seconds_per_form_and_turn=seconds,
               reads_with_three_hits=int((per_read == 3).sum()), reads_found_by_scan=int(found.sum()), **counts)
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 4) for x in v]
    rec["b_over_a"] = [round(min(ms["b"]) / max(ms["a"]), 3), round(max(ms["b"]) / min(ms["a"]), 3)]      # the range over the turns
    rec["a_config"], rec["b_config"] = last["a_cfg"], cfg
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "edit_scan_hits_rate.jsonl"))
    arg = ap.parse_args()
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    for seed, nq, l1 in ((21, 4096, 150), (22, 1024, 1000)):
        line = json.dumps(measure(seed, nq, l1, arg.turns, arg.seconds))
        print(line, flush=True)
        with open(arg.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
