#!/usr/bin/env python3
"""edit_infix_rate.py -- what edit infix mode (at_set_edit_infix) costs beside the global edit distance, on one GPU from host memory;
one JSON line per workload.

    python3 tools/edit_infix_rate.py [--reps 3] [--only a|b|c] [--no-search] [--no-device] [--out FILE]

Pairs: 100 000 reads of 150 bases, each planted in its own window of 500 with 4 % substitutions and a deletion of three bases in
every fourth.  Three forms, each warmed up once, then taking turns `reps` times:
    a   edit -u 1, global, the number only   (the untouched at_myers path: the yardstick)
    b   infix, the number only               (at_set_edit_infix, at_align_batch, want_traceback = 0)
    c   infix with ops                       (at_set_edit_infix + at_set_edit_traceback, at_align_batch)
Search: 20 000 such reads against 200 windows of 500, k = 1, both strands, infix (at_search_strands): 8 000 000 pairs.
Device: the same 100 000 pairs resident in device memory, the three forms through at_align_batch_device, 20 launches each timed with
events (milliseconds per launch, best and median) -- the kernels alone, which the host rows hide behind the transfers.
Seconds are end-to-end per call; GCUPS = pairs * l1 * l2 / seconds / 1e9.  The ratios use the best repetition of each form.
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

L1, L2 = 150, 500
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def planted(rng, windows, which):
    """one read per entry of `which`: 150 bases of windows[which[k]] from a random start, 4 % substituted, three bases deleted in every
    fourth (the read is refilled from the window behind it)"""
    n = len(which)
    at = rng.integers(0, L2 - L1 - 3, size=n)
    reads = windows[which[:, None], at[:, None] + np.arange(L1 + 3)[None, :]]
    for k in range(0, n, 4):
        cut = int(rng.integers(20, L1 - 20))
        reads[k, cut:L1] = reads[k, cut + 3:L1 + 3].copy()
    reads = reads[:, :L1].copy()
    sub = rng.random((n, L1)) < 0.04
    reads[sub] = ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    return reads


def measure_pairs(n, reps, only):
    rng = np.random.default_rng(7)
    windows = ACGT[rng.integers(0, 4, size=(n, L2))]
    reads = planted(rng, windows, np.arange(n))
    blob = np.concatenate([np.concatenate([reads, windows], axis=1).reshape(-1), np.zeros(64, dtype=np.uint8)])
    off1 = np.arange(n, dtype=np.int64) * (L1 + L2)
    off2 = off1 + L1
    len1, len2 = np.full(n, L1, dtype=np.int32), np.full(n, L2, dtype=np.int32)
    al = A.Aligner(0)
    al.set_scoring(1, 1, -5, -1, -10)
    lib, h, p = al._lib, al._h, A._ptr
    score, ei, ej, st, cnt = (np.zeros(n, dtype=np.int32) for _ in range(5))
    slot = np.arange(n, dtype=np.int64) * (L1 + L2)
    ops = np.zeros(n * (L1 + L2) + 64, dtype=np.uint8)
    cfg, check = {}, {}

    def run(form):
        al.set_edit_infix(form in "bc")
        al.set_edit_traceback(form == "c")
        tb = form == "c"
        t0 = time.perf_counter()
        rc = lib.at_align_batch(h, A.MODE_EDIT, n, p(blob), p(off1), p(len1), p(off2), p(len2), 1 if tb else 0, p(score), p(ei), p(ej), p(st),
                                p(ops) if tb else None, p(slot) if tb else None, p(cnt) if tb else None)
        dt = time.perf_counter() - t0
        al._check(rc)
        cfg[form] = al.last_config
        check[form] = (int(score.astype(np.int64).sum()), int(ej.astype(np.int64).sum()))
        return dt

    forms = [only] if only else ["a", "b", "c"]
    for f in forms:
        run(f)                                                              # warm-up: buffers grown, payload sizes learnt
    times = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            times[f].append(run(f))
    al.close()
    rec = dict(what="edit infix: %d reads of %d planted in windows of %d, from host memory" % (n, L1, L2), pairs=n, l1=L1, l2=L2, reps=reps)
    for f in forms:
        rec[f + "_s"] = [round(x, 5) for x in times[f]]
        rec[f + "_gcups"] = round(n * L1 * L2 / min(times[f]) / 1e9, 1)
        rec[f + "_score_sum"], rec[f + "_end_j_sum"] = check[f]
        rec[f + "_config"] = cfg[f]
    if not only:
        assert check["b"] == check["c"] and check["a"][1] == n * L2 and check["b"][0] < check["a"][0], check
        rec["b_over_a"] = round(min(times["b"]) / min(times["a"]), 2)
        rec["c_over_b"] = round(min(times["c"]) / min(times["b"]), 2)
    return rec


def measure_device(n, launches=20):
    import torch
    rng = np.random.default_rng(7)
    windows = ACGT[rng.integers(0, 4, size=(n, L2))]
    reads = planted(rng, windows, np.arange(n))
    words, woff1, woff2, len1, len2, bits = A.pack_pairs([(bytes(r), bytes(w)) for r, w in zip(reads, windows)])
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("w", words.view(np.int32)), ("o1", woff1), ("o2", woff2), ("l1", len1), ("l2", len2))}
    out = torch.zeros((5, n), dtype=torch.int32, device=dev)
    ops = torch.zeros(n * (L1 + L2) + 64, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(np.arange(n, dtype=np.int64) * (L1 + L2)).to(dev)
    al = A.Aligner(0)
    al.set_scoring(1, 1, -5, -1, -10)
    stream = torch.cuda.current_stream().cuda_stream
    rec = dict(what="edit infix, kernels alone: %d pairs of %dx%d resident in device memory" % (n, L1, L2), pairs=n, l1=L1, l2=L2, launches=launches)
    best = {}
    for form in "abc":
        al.set_edit_infix(form in "bc")
        al.set_edit_traceback(form == "c")

        def launch():
            al.align_batch_device(A.MODE_EDIT, n, d["w"].data_ptr(), bits, d["o1"].data_ptr(), d["l1"].data_ptr(), d["o2"].data_ptr(),
                                  d["l2"].data_ptr(), L1, L2, False, form == "c", out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                  out[3].data_ptr(), ops.data_ptr(), d_off.data_ptr(), out[4].data_ptr(), stream)
        launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        best[form] = min(ms)
        rec[form + "_ms_best"], rec[form + "_ms_median"] = round(min(ms), 4), round(float(np.median(ms)), 4)
        rec[form + "_tcups"] = round(n * L1 * L2 / min(ms) / 1e9, 2)
        rec[form + "_score_sum"] = int(out[0].sum(dtype=torch.int64).item())
        rec[form + "_config"] = al.last_config
    al.close()
    rec["b_over_a"], rec["c_over_b"] = round(best["b"] / best["a"], 2), round(best["c"] / best["b"], 2)
    return rec


def measure_search(nq, nt, reps):
    rng = np.random.default_rng(8)
    windows = ACGT[rng.integers(0, 4, size=(nt, L2))]
    home = rng.integers(0, nt, size=nq)
    reads = planted(rng, windows, home)
    queries = [bytes(r) for r in reads]
    for k in range(1, nq, 2):                                               # every other read lies on the other strand
        queries[k] = A.revcomp(queries[k])
    targets = [bytes(w) for w in windows]
    al = A.Aligner(0)
    al.set_scoring(1, 1, -5, -1, -10)
    al.set_edit_infix(True)
    times, hits = [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        hits = al.search("edit", queries, targets, k=1, strands="both")
        if r:
            times.append(time.perf_counter() - t0)
    cfg = al.last_config
    al.close()
    found = int(((hits["target"][:, 0] == home) & (hits["strand"][:, 0] == np.arange(nq) % 2)).sum())
    pairs = 2 * nq * nt
    return dict(what="edit infix search: %d reads of %d x %d windows of %d, k=1, both strands" % (nq, L1, nt, L2), queries=nq, targets=nt,
                pairs=pairs, reps=reps, s=[round(x, 5) for x in times], gcups=round(pairs * L1 * L2 / min(times) / 1e9, 1),
                reads_at_home=found, score_sum=int(hits["score"][:, 0].astype(np.int64).sum()), config=cfg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["a", "b", "c"])
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--out", default=None)
    arg = ap.parse_args()
    recs = [measure_pairs(100000, arg.reps, arg.only)]
    if not arg.no_search and not arg.only:
        recs.append(measure_search(20000, 200, arg.reps))
    if not arg.no_device and not arg.only:
        recs.append(measure_device(100000))
    for rec in recs:
        line = json.dumps(rec)
        print(line, flush=True)
        if arg.out:
            with open(arg.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
