#!/usr/bin/env python3
"""allpairs_hits_rate.py -- what at_allpairs_hits (all-vs-all of which only the pairs over a threshold leave the device)
costs beside the dense thresholded run it replaces, on one GPU; one JSON line, appended to profiles/r13/allpairs_hits_rate.jsonl.

    python3 tools/allpairs_hits_rate.py [--reads 12000] [--turns 3] [--out FILE]

Read set: `reads` reads of 1 000 bases cut at random places of one seeded random genome of reads * 333 bases, each with 1 %
substitutions: about 6 of 10 000 pairs truly overlap.  Overlap mode, scoring 1 / -2 / -5 / -1, threshold 30 (the C5 test's).  Three
forms, each warmed up once, then taking turns; a turn is ONE call (seconds at the default size), wall clock around a call that ends
synchronised:
    a   the dense way: at_align_allpairs_stream with at_set_min_score(threshold), the callback picking the pairs over the threshold out
        of every slice with numpy
    b   at_allpairs_hits, scores only
    c   at_allpairs_hits with CIGARs
The three forms' kept pairs are compared (they must be equal) before anything is written."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aligntools.c_amd as A  # noqa: E402

L, T = 1000, 30
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_reads(seed, n):
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=n * 333)
    at = rng.integers(0, len(genome) - L, size=n)
    codes = genome[at[:, None] + np.arange(L)[None, :]]
    sub = rng.random(codes.shape) < 0.01
    codes[sub] = (codes[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
    blob = np.concatenate([ACGT[codes].reshape(-1), np.zeros(64, dtype=np.uint8)])
    return blob, np.arange(n, dtype=np.int64) * L, np.full(n, L, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=12000)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "allpairs_hits_rate.jsonl"))
    arg = ap.parse_args()
    n = arg.reads
    total = n * (n - 1) // 2
    blob, off, lens = make_reads(0xA11, n)
    al = A.Aligner(0)
    al.set_scoring(1, -2, -5, -1)
    p = A._ptr
    cfg, res = {}, {}

    def form_a():
        got = []

        def on_slice(first, sc, ei, ej, st):
            idx = np.nonzero((st != 0) & (sc >= T))[0]
            got.append((first + idx, sc[idx], ei[idx], ej[idx], st[idx]))
        al.set_min_score(T)
        t0 = time.perf_counter()
        al.align_allpairs_stream("overlap", blob, off, lens, 0, total, 0, on_slice)
        dt = time.perf_counter() - t0
        al.set_min_score(None)
        cfg["a"] = al.last_config
        res["a"] = [np.concatenate(x) for x in zip(*got)]
        return dt

    cap = {"hits": 1 << 16, "words": 1 << 20}

    def hits_call(cigar):
        for _ in range(3):                                     # (the warm-up finds the capacities; the timed calls are one call each)
            k = cap["hits"]
            pair = np.zeros(k, dtype=np.int64)
            o = [np.zeros(k, dtype=np.int32) for _ in range(6)]
            stats = np.zeros((k, 8), dtype=np.int32) if cigar else None
            ncg = np.zeros(k, dtype=np.int32) if cigar else None
            coff = np.zeros(k + 1, dtype=np.int64) if cigar else None
            words = np.zeros(cap["words"], dtype=np.uint32) if cigar else None
            nh = C.c_int64(0)
            t0 = time.perf_counter()
            rc = al._lib.at_allpairs_hits(al._h, A.MODE_OVERLAP, n, p(blob), p(off), p(lens), 0, total, T, 0, 0, k, C.addressof(nh), p(pair),
                                          *[p(x) for x in o], p(stats), p(ncg), p(coff), p(words), cap["words"] if cigar else 0)
            dt = time.perf_counter() - t0
            al._check(rc)
            if nh.value > k:
                cap["hits"] = int(nh.value) + 1024
                continue
            if cigar and coff[nh.value] > cap["words"]:
                cap["words"] = int(coff[nh.value]) + 1024
                continue
            break
        else:
            raise RuntimeError("the capacities did not settle")
        which = "c" if cigar else "b"
        cfg[which] = al.last_config
        h = int(nh.value)
        res[which] = [pair[:h], o[2][:h], o[3][:h], o[4][:h], o[5][:h]]
        if cigar:
            res["words"] = int(coff[h])
        return dt

    form_a(); hits_call(False); hits_call(True)                # warm-up of each form (and the capacities of b and c)
    sec = {k: [] for k in "abc"}
    for _ in range(arg.turns):
        sec["a"].append(form_a())
        sec["b"].append(hits_call(False))
        sec["c"].append(hits_call(True))
    for which in "bc":
        for x, y in zip(res["a"], res[which]):
            assert np.array_equal(x, y), "form %s does not keep what the dense run keeps" % which
    al.close()
    med = {k: float(np.median(v)) for k, v in sec.items()}
    rec = dict(what="all-vs-all overlap of %d reads of %d bases (%d pairs), scoring 1/-2/-5/-1, threshold %d: dense thresholded stream + numpy "
                    "filter (a), at_allpairs_hits (b), with CIGARs (c); wall seconds per call" % (n, L, total, T),
               reads=n, pairs=total, threshold=T, turns=arg.turns, kept=int(len(res["a"][0])), cigar_words=res["words"],
               a_s=[round(x, 4) for x in sec["a"]], b_s=[round(x, 4) for x in sec["b"]], c_s=[round(x, 4) for x in sec["c"]],
               a_median_s=round(med["a"], 4), b_median_s=round(med["b"], 4), c_median_s=round(med["c"], 4),
               a_spread_s=round(max(sec["a"]) - min(sec["a"]), 4), b_minus_a_s=round(med["b"] - med["a"], 4),
               b_within_a_spread=bool(med["b"] - med["a"] <= max(sec["a"]) - min(sec["a"])),
               a_config=cfg["a"], b_config=cfg["b"], c_config=cfg["c"], kernel_source_sha16=A.kernel_source_sha16())
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    with open(arg.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
