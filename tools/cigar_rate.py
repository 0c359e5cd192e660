#!/usr/bin/env python3
"""cigar_rate.py -- the three traceback forms of the host entry side by side on one GPU; one JSON line per measurement.

    python3 tools/cigar_rate.py [--pairs 100000] [--len 150] [--reps 3] [--kind unrelated|related] [--only ops|strings|cigar] [--out FILE]

100 000 local pairs of 150 x 150 bases from host memory through at_align_batch (op codes), at_align_batch_strings (the two gapped
strings) and at_align_batch_cigar (statistics rows + run-length CIGAR words): end-to-end seconds of each call, the three taking
turns `reps` times after a warm-up of each, and the bytes per pair that come down from the device behind the five fixed-size
result arrays (20 bytes per pair in all three forms):
    ops       nops bytes + the 8-byte offset
    strings   2 (nops + 1) bytes + the 8-byte offset
    cigar     4 bytes per run + the 32-byte statistics row + the 4-byte run count + the 8-byte offset
--kind related: the second read is the first with 4 % substitutions and an indel in every fourth pair (a mapper's hits: alignments
as long as the reads); unrelated: two random reads (alignments of a dozen columns).
Kernel shares: `rocprofv3 --kernel-trace --stats -- python3 tools/cigar_rate.py --only cigar` (tools/README.md).
"""
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


def make_pairs(rng, n, length, kind):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = acgt[rng.integers(0, 4, size=(n, length))]
    if kind == "unrelated":
        b = acgt[rng.integers(0, 4, size=(n, length))]
    else:
        b = a.copy()
        sub = rng.random((n, length)) < 0.04
        b[sub] = acgt[rng.integers(0, 4, size=int(sub.sum()))]
        for k in range(0, n, 4):                                            # a deletion of three bases, the tail refilled
            at = int(rng.integers(20, length - 20))
            b[k, at:length - 3] = b[k, at + 3:].copy()
            b[k, length - 3:] = acgt[rng.integers(0, 4, size=3)]
    blob = np.concatenate([a, b], axis=1).reshape(-1).copy()
    blob = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
    off1 = np.arange(n, dtype=np.int64) * (2 * length)
    lens = np.full(n, length, dtype=np.int32)
    return blob, off1, lens, off1 + length, lens.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kind", default="unrelated", choices=["unrelated", "related"])
    ap.add_argument("--only", default=None, choices=["ops", "strings", "cigar"])
    ap.add_argument("--out", default=None)
    arg = ap.parse_args()
    n, L = arg.pairs, arg.len
    al = A.Aligner(0)
    al.set_scoring(1, -2, -5, -1, -10)
    lib, h, p = al._lib, al._h, A._ptr
    blob, off1, len1, off2, len2 = make_pairs(np.random.default_rng(7), n, L, arg.kind)
    score, ei, ej, st, cnt = (np.zeros(n, dtype=np.int32) for _ in range(5))
    slot = np.arange(n, dtype=np.int64) * (2 * L + 1)
    buf1 = np.zeros(n * (2 * L + 1) + 64, dtype=np.uint8)
    buf2 = np.zeros(n * (2 * L + 1) + 64, dtype=np.uint8)
    stats = np.zeros((n, 8), dtype=np.int32)
    cgoff = np.zeros(n + 1, dtype=np.int64)
    words = np.zeros(n * 2 * L, dtype=np.uint32)
    cfg, payload = {}, {}

    def run(form):
        t0 = time.perf_counter()
        if form == "ops":
            rc = lib.at_align_batch(h, A.MODE_LOCAL, n, p(blob), p(off1), p(len1), p(off2), p(len2), 1, p(score), p(ei), p(ej), p(st),
                                    p(buf1), p(slot), p(cnt))
        elif form == "strings":
            rc = lib.at_align_batch_strings(h, A.MODE_LOCAL, n, p(blob), p(off1), p(len1), p(off2), p(len2), p(score), p(ei), p(ej), p(st),
                                            p(buf1), p(buf2), p(slot), p(cnt))
        else:
            rc = lib.at_align_batch_cigar(h, A.MODE_LOCAL, n, p(blob), p(off1), p(len1), p(off2), p(len2), 0, p(score), p(ei), p(ej), p(st),
                                          p(stats), p(cnt), p(cgoff), p(words), len(words))
        dt = time.perf_counter() - t0
        al._check(rc)
        cfg[form] = al.last_config
        total = float(cnt.sum())
        payload[form] = {"ops": total / n + 8, "strings": 2 * (total / n + 1) + 8, "cigar": 4 * total / n + 32 + 4 + 8}[form]
        return dt

    forms = [arg.only] if arg.only else ["ops", "strings", "cigar"]
    for f in forms:
        run(f)                                                              # warm-up: buffers grown, payload sizes learnt
    times = {f: [] for f in forms}
    for _ in range(arg.reps):
        for f in forms:
            times[f].append(run(f))
    rec = dict(what="local %dx%d, %d %s pairs from host memory, tracebacks in three forms" % (L, L, n, arg.kind), pairs=n, reps=arg.reps,
               kind=arg.kind)
    for f in forms:
        rec[f + "_s"] = [round(x, 5) for x in times[f]]
        rec[f + "_payload_bytes_per_pair"] = round(payload[f], 2)
        rec[f + "_config"] = cfg[f]
    if not arg.only:
        rec["mean_columns_per_pair"] = round(payload["ops"] - 8, 2)
        rec["mean_runs_per_pair"] = round((payload["cigar"] - 44) / 4, 2)
    line = json.dumps(rec)
    print(line, flush=True)
    if arg.out:
        with open(arg.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
