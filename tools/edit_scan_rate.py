#!/usr/bin/env python3
"""edit_scan_rate.py -- what at_scan (reads against long targets) costs beside the same tiles swept as explicit pairs by
the infix kernel, on one GPU; one JSON line per read set, appended to profiles/r11/edit_scan_rate.jsonl.

    python3 tools/edit_scan_rate.py [--turns 3] [--seconds 1.0] [--out FILE]

Read sets: 4 096 reads of 150 bases and 1 024 reads of 1 000 bases, each planted (4 % substitutions, a deletion of three bases in
every fourth, every other read reverse-complemented -- those stay unfound on the forward strand) in one seeded target of 300 000
bases.  Three forms, each warmed up once, then taking turns; within a turn a form is repeated until `seconds` have passed:
    a   the baseline: tiles with their overlap as explicit pairs resident in device memory, through at_align_batch_device under
        at_set_edit_infix, number only -- the kernel at_infix<W, false>; events around each launch.  Its tiles are the default
        width's where T + ov <= 3 792 columns, else the widest that fit (Ta), and form b is then also run at Ta
    b   the sweep phase of at_scan (key slots, at_scan<W>, unpack, merge), the device time at_last_config reports as sweep=..ms;
        also at other tile widths, against the sweep efficiency T / (T + ov)
    c   at_scan end to end from host memory, without and with CIGARs (wall clock)
TCUPS counts the USEFUL cells, reads x l1 x l2, for every form: form a and b sweep (T + ov) / T times as many.
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
WIDTHS = (256, 512, 1024, 2048, 4096)


def make_set(seed, nq, l1):
    rng = np.random.default_rng(seed)
    target = ACGT[rng.integers(0, 4, size=L2)]
    at = rng.integers(0, L2 - l1 - 3, size=nq)
    reads = target[at[:, None] + np.arange(l1 + 3)[None, :]]
    for k in range(0, nq, 4):
        cut = int(rng.integers(20, l1 - 20))
        reads[k, cut:l1] = reads[k, cut + 3:l1 + 3].copy()
    reads = reads[:, :l1].copy()
    sub = rng.random((nq, l1)) < 0.04
    reads[sub] = ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    queries = [bytes(r) for r in reads]
    for k in range(1, nq, 2):
        queries[k] = A.revcomp(queries[k])
    return queries, bytes(target)


def until(seconds, fn):
    """fn() -> a figure; repeated until `seconds` have passed; the figures"""
    out, t0 = [], time.perf_counter()
    while not out or time.perf_counter() - t0 < seconds:
        out.append(fn())
    return out


def measure(seed, nq, l1, turns, seconds):
    import torch
    queries, target = make_set(seed, nq, l1)
    cells = nq * l1 * L2
    T, ov, groups = A.scan_plan(l1, L2)
    Ta = min(T, (3792 - ov) & ~15)                                         # the baseline's bound: 64 LDS windows of T + ov columns
    # ---- form a: the same tiles as explicit pairs, descriptors built here, sequences packed once
    words, woff1, woff2, _len1, _len2, bits = A.pack_pairs([(queries[0], target)] + [(q, b"") for q in queries[1:]])
    assert bits == 2
    ntile = -(-L2 // Ta)
    s0 = np.maximum(0, np.arange(ntile, dtype=np.int64) * Ta - ov)
    e = np.minimum((np.arange(ntile, dtype=np.int64) + 1) * Ta, L2)
    pw1 = np.repeat(woff1, ntile)
    pw2 = np.tile(woff2[0] + s0 // 16, nq)
    pl1 = np.full(nq * ntile, l1, dtype=np.int32)
    pl2 = np.tile((e - s0).astype(np.int32), nq)
    npairs = nq * ntile
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("w", words.view(np.int32)), ("o1", pw1), ("o2", pw2), ("l1", pl1), ("l2", pl2))}
    out = torch.zeros((4, npairs), dtype=torch.int32, device=dev)
    base = A.Aligner(0)
    base.set_scoring(1, 1, -5, -1, -10)
    base.set_edit_infix(True)
    stream = torch.cuda.current_stream().cuda_stream

    def form_a():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        base.align_batch_device(A.MODE_EDIT, npairs, d["w"].data_ptr(), bits, d["o1"].data_ptr(), d["l1"].data_ptr(), d["o2"].data_ptr(),
                                d["l2"].data_ptr(), l1, Ta + ov, False, False, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                out[3].data_ptr(), 0, 0, 0, stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    al = A.Aligner(0)
    al.set_scoring(1, 1, -5, -1, -10)
    hits = {}

    def form_b(tile_cols=0):
        hits["b"] = al.scan(queries, [target], tile_cols=tile_cols)
        return float(al.last_config.rsplit("sweep=", 1)[1].split("ms")[0])

    def form_c(cigar):
        t0 = time.perf_counter()
        hits["c"] = al.scan(queries, [target], cigar=cigar)
        return (time.perf_counter() - t0) * 1e3

    form_a(); form_b(); form_c(False); form_c(True)                      # warm-up of each form
    cfg_a, cfg_b = base.last_config, al.last_config.rsplit(" sweep=", 1)[0]
    # the baseline's minimum over a read's tiles is the scan's score wherever the scan is exact (every read here: no cutoff)
    a_score = out[0].view(nq, ntile).min(dim=1).values.cpu().numpy()
    assert np.array_equal(a_score, hits["b"]["score"][:, 0]), "form a and form b disagree"
    ms = {k: [] for k in ("a", "b", "c", "c_cigar")}
    for _ in range(turns):
        ms["a"].append(float(np.median(until(seconds, form_a))))
        ms["b"].append(float(np.median(until(seconds, form_b))))
        ms["c"].append(float(np.median(until(seconds, lambda: form_c(False)))))
        ms["c_cigar"].append(float(np.median(until(seconds, lambda: form_c(True)))))
    widths = {}
    for w in sorted(set(WIDTHS + (Ta,))):
        form_b(w)
        _t, ov_w, g_w = A.scan_plan(l1, L2, None, w)
        widths[str(w)] = dict(ms=round(float(np.median(until(seconds / 2, lambda: form_b(w)))), 4), groups=g_w, efficiency=round(w / (w + ov_w), 3))
    found = int((hits["c"]["score"][:, 0] <= l1 // 8).sum())
    base.close(); al.close()
    rec = dict(what="scan: %d reads of %d in one target of %d, forward strand, k=1" % (nq, l1, L2), reads=nq, l1=l1, l2=L2, tile=T, baseline_tile=Ta, overlap=ov,
               groups=groups, tiles_as_pairs=npairs, turns=turns, seconds_per_form_and_turn=seconds,
               reads_found=found, score_sum=int(hits["c"]["score"][:, 0].astype(np.int64).sum()))
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 4) for x in v]
        rec[k + "_tcups"] = round(cells / min(v) / 1e9, 2)
    rec["b_over_a"] = [round(min(ms["b"]) / max(ms["a"]), 3), round(max(ms["b"]) / min(ms["a"]), 3)]      # the range over the turns
    rec["b_widths"] = widths
    rec["a_config"], rec["b_config"] = cfg_a, cfg_b
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "edit_scan_rate.jsonl"))
    arg = ap.parse_args()
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    for seed, nq, l1 in ((11, 4096, 150), (12, 1024, 1000)):
        line = json.dumps(measure(seed, nq, l1, arg.turns, arg.seconds))
        print(line, flush=True)
        with open(arg.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
