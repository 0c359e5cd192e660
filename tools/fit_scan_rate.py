#!/usr/bin/env python3
"""fit_scan_rate.py -- what at_scan_fit (end-to-end affine alignment of reads against long targets) costs beside
at_search in fit mode on the same inputs, on one GPU; one JSON line per read set and cutoff, appended to
profiles/r20/fit_scan_rate.jsonl.

    python3 tools/fit_scan_rate.py [--turns 3] [--seconds 1.0] [--baseline-reads 64] [--out FILE]

Read sets: 4 096 reads of 150 bases and 1 024 reads of 1 000 bases, each planted (4 % substitutions, a deletion of three bases in
every fourth) in one seeded target of 300 000 bases; scoring 2/-2/-5/-2, forward strand, k = 1.  Per set one row with a min_score of
half the perfect score (the headline) and one without a cutoff, where the overlap is at its widest.  Three forms, each warmed up
once, then taking turns; within a turn a form is repeated until `seconds` have passed:
    a   the baseline: Aligner.search("fit") with the whole target per pair (at_search; its code is the parent commit's, this change
        does not touch it), wall clock.  It runs on the first --baseline-reads reads and its time is SCALED to the whole set
        (reads / baseline reads): the scaled figure is marked as such
    b   the sweep phase of at_scan_fit (descriptors, the batch entry's sweep, fold, unpack, merge of every slice), the device time
        between two events that at_last_config reports as sweep=..ms; also at other tile widths, each with its at_last_config: fit's
        values drift downward, so which kernel family takes a tile depends on its length T + ov
    c   at_scan_fit end to end from host memory, without and with CIGARs (wall clock)
Before any time is written the lists of a (on its reads) and c must be identical.  TCUPS counts the USEFUL cells, reads x l1 x l2.
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

L2 = 300000
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
WIDTHS = (256, 512, 1024, 2048)
SCORING = (2, -2, -5, -2)


def make_set(seed, nq, l1):
    rng = np.random.default_rng(seed)
    target = ACGT[rng.integers(0, 4, size=L2)]
    at = rng.integers(0, L2 - l1 - 4, size=nq)
    reads = target[at[:, None] + np.arange(l1 + 3)[None, :]]
    for k in range(0, nq, 4):
        cut = int(rng.integers(20, l1 - 20))
        reads[k, cut:l1] = reads[k, cut + 3:l1 + 3].copy()
    reads = reads[:, :l1].copy()
    sub = rng.random((nq, l1)) < 0.04
    reads[sub] = ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    return [bytes(r) for r in reads], bytes(target)


def until(seconds, fn):
    """fn() -> a figure; repeated until `seconds` have passed; the figures"""
    out, t0 = [], time.perf_counter()
    while not out or time.perf_counter() - t0 < seconds:
        out.append(fn())
    return out


def measure(seed, nq, l1, min_score, turns, seconds, nbase):
    queries, target = make_set(seed, nq, l1)
    cells = nq * l1 * L2
    T, ov, ntiles, _nfull = A.scan_fit_plan(l1, L2, *SCORING, min_score=min_score)
    al = A.Aligner(0)
    al.set_scoring(*SCORING)
    hits = {}

    def form_a():
        t0 = time.perf_counter()
        hits["a"] = al.search("fit", queries[:nbase], [target], cutoff=min_score)
        return (time.perf_counter() - t0) * 1e3 * (nq / nbase)

    def form_b(tile_cols=0):
        hits["b"] = al.scan_fit(queries, [target], min_score=min_score, tile_cols=tile_cols)
        return float(al.last_config.rsplit("sweep=", 1)[1].split("ms")[0])

    def form_c(cigar):
        t0 = time.perf_counter()
        hits["c"] = al.scan_fit(queries, [target], min_score=min_score, cigar=cigar)
        return (time.perf_counter() - t0) * 1e3

    form_a()
    cfg_a = al.last_config
    form_b()
    cfg_b = al.last_config.rsplit(" sweep=", 1)[0]
    form_c(True); form_c(False)                                         # warm-up of each form
    for name in ("target", "score", "end_i", "end_j", "state", "nhits"):
        assert np.array_equal(hits["a"][name], hits["c"][name][:nbase]), "form a and form c disagree in " + name
    ms = {k: [] for k in ("a", "b", "c", "c_cigar")}
    for _ in range(turns):
        ms["a"].append(float(np.median(until(seconds, form_a))))
        ms["b"].append(float(np.median(until(seconds, form_b))))
        ms["c"].append(float(np.median(until(seconds, lambda: form_c(False)))))
        ms["c_cigar"].append(float(np.median(until(seconds, lambda: form_c(True)))))
    widths = {}
    for w in WIDTHS:
        form_b(w)
        cfg_w = al.last_config.rsplit(" sweep=", 1)[0]
        _t, ov_w, n_w, _f = A.scan_fit_plan(l1, L2, *SCORING, min_score=min_score, tile_cols=w)
        widths[str(w)] = dict(ms=round(float(np.median(until(seconds / 2, lambda: form_b(w)))), 4), tiles=n_w, efficiency=round(w / (w + ov_w), 3), config=cfg_w)
    found = int((hits["c"]["nhits"] > 0).sum())
    al.close()
    rec = dict(what="fit scan: %d reads of %d in one target of %d, forward strand, k=1, scoring 2/-2/-5/-2, min_score=%s" % (nq, l1, L2, min_score),
               reads=nq, l1=l1, l2=L2, min_score=min_score, tile=T, overlap=ov, tiles=ntiles, efficiency=round(T / (T + ov), 3), turns=turns,
               seconds_per_form_and_turn=seconds, baseline_reads=nbase, a_is_scaled_by=round(nq / nbase, 3), reads_with_a_hit=found,
               score_sum=int(hits["c"]["score"][:, 0].astype(np.int64).sum()), kernel_source_sha16=A.kernel_source_sha16())
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 4) for x in v]
        rec[k + "_tcups"] = round(cells / min(v) / 1e9, 3)
    rec["b_over_a"] = [round(min(ms["b"]) / max(ms["a"]), 4), round(max(ms["b"]) / min(ms["a"]), 4)]      # the range over the turns
    rec["b_below_a_in_every_turn"] = all(b < a for a, b in zip(ms["a"], ms["b"]))
    rec["b_widths"] = widths
    rec["a_config"], rec["b_config"] = cfg_a, cfg_b
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--baseline-reads", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "fit_scan_rate.jsonl"))
    arg = ap.parse_args()
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    for seed, nq, l1 in ((11, 4096, 150), (12, 1024, 1000)):
        for min_score in (l1, None):                                    # half the perfect score of 2 * l1; no cutoff
            line = json.dumps(measure(seed, nq, l1, min_score, arg.turns, arg.seconds, min(arg.baseline_reads, nq)))
            print(line, flush=True)
            with open(arg.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
