#!/usr/bin/env python3
"""edit_align_rate.py -- what the alignment behind an edit distance costs, on one GPU from host memory; one JSON line per workload.

    python3 tools/edit_align_rate.py [--reps 3] [--only a|b|c|d] [--shape 150|1000] [--out FILE]

Two workloads of related pairs (the second read is the first with 4 % substitutions and an indel in every fourth pair): 100 000
pairs of 150 x 150 and 20 000 pairs of 1000 x 1000.  Four forms, each warmed up once, then taking turns `reps` times:
    a   edit -u 1, the number only                      (at_align_batch, want_traceback = 0)
    b   edit -u 1 with ops                              (at_set_edit_traceback, at_align_batch)
    c   edit -u 1 with CIGARs and statistics rows       (at_set_edit_traceback, at_align_batch_cigar)
    d   global m=0 u=-1 o=-1 e=-1 with ops on the same pairs: the nearest thing there was before.  Its results are NOT edit's
        (the reference's border row costs o + e k, an interior gap o + e (k - 1)); it is here for the time only.
Seconds are end-to-end per call; GCUPS = pairs * l1 * l2 / seconds / 1e9.  The ratios b/a and b/d use the best repetition of each.
Kernel shares: `rocprofv3 --kernel-trace --stats -- python3 tools/edit_align_rate.py --only b` (tools/README.md).
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
from cigar_rate import make_pairs  # noqa: E402

WORKLOADS = {150: 100000, 1000: 20000}


def measure(n, L, reps, only):
    al = A.Aligner(0)
    lib, h, p = al._lib, al._h, A._ptr
    blob, off1, len1, off2, len2 = make_pairs(np.random.default_rng(7), n, L, "related")
    score, ei, ej, st, cnt = (np.zeros(n, dtype=np.int32) for _ in range(5))
    slot = np.arange(n, dtype=np.int64) * (2 * L)
    ops = np.zeros(n * 2 * L + 64, dtype=np.uint8)
    stats = np.zeros((n, 8), dtype=np.int32)
    cgoff = np.zeros(n + 1, dtype=np.int64)
    words = np.zeros(n * 2 * L, dtype=np.uint32)
    cfg, check = {}, {}

    def run(form):
        if form == "d":
            al.set_scoring(0, -1, -1, -1, -10)
        else:
            al.set_scoring(1, 1, -5, -1, -10)
        al.set_edit_traceback(form in "bc")
        t0 = time.perf_counter()
        if form == "a":
            rc = lib.at_align_batch(h, A.MODE_EDIT, n, p(blob), p(off1), p(len1), p(off2), p(len2), 0, p(score), p(ei), p(ej), p(st), None, None, None)
        elif form == "b":
            rc = lib.at_align_batch(h, A.MODE_EDIT, n, p(blob), p(off1), p(len1), p(off2), p(len2), 1, p(score), p(ei), p(ej), p(st), p(ops), p(slot), p(cnt))
        elif form == "c":
            rc = lib.at_align_batch_cigar(h, A.MODE_EDIT, n, p(blob), p(off1), p(len1), p(off2), p(len2), 0, p(score), p(ei), p(ej), p(st),
                                          p(stats), p(cnt), p(cgoff), p(words), len(words))
        else:
            rc = lib.at_align_batch(h, A.MODE_GLOBAL, n, p(blob), p(off1), p(len1), p(off2), p(len2), 1, p(score), p(ei), p(ej), p(st), p(ops), p(slot), p(cnt))
        dt = time.perf_counter() - t0
        al._check(rc)
        cfg[form] = al.last_config
        check[form] = int(score.astype(np.int64).sum())
        return dt

    forms = [only] if only else ["a", "b", "c", "d"]
    for f in forms:
        run(f)                                                              # warm-up: buffers grown, payload sizes learnt
    times = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            times[f].append(run(f))
    al.close()
    rec = dict(what="edit alignments: %d related pairs of %dx%d from host memory" % (n, L, L), pairs=n, len=L, reps=reps)
    for f in forms:
        rec[f + "_s"] = [round(x, 5) for x in times[f]]
        rec[f + "_gcups"] = round(n * L * L / min(times[f]) / 1e9, 1)
        rec[f + "_score_sum"] = check[f]
        rec[f + "_config"] = cfg[f]
    if not only:
        assert check["a"] == check["b"] == check["c"], check
        rec["b_over_a"] = round(min(times["b"]) / min(times["a"]), 2)
        rec["b_over_d"] = round(min(times["b"]) / min(times["d"]), 2)
        rec["c_over_b"] = round(min(times["c"]) / min(times["b"]), 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["a", "b", "c", "d"])
    ap.add_argument("--shape", type=int, default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=None)
    arg = ap.parse_args()
    for L in ([arg.shape] if arg.shape else sorted(WORKLOADS)):
        line = json.dumps(measure(WORKLOADS[L], L, arg.reps, arg.only))
        print(line, flush=True)
        if arg.out:
            with open(arg.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
