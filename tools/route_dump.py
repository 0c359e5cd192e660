"""Which kernel family, group width, rows per lane and storage class a fixed list of small batches takes: one JSON line per case
with at_last_config, to compare two builds of the library on one card (`AT_LIB_PATH=... route_dump.py OUT.jsonl`; grids depend on
the card).  Under a minute:

    uniform 150 x 150 and 1024 x 1024 in every mode (fit also with -s), 20 000 and 600 pairs, two scorings, with tracebacks
    ragged: the read lengths around every row-class edge (the lists of tests/test_gpu_parity.py: local, global / fit, long reads),
            1 400 pairs each, local / global / fit / fit -s / overlap with tracebacks, ACGT and ACGT + N
    edit at 64 / 160 / 1 000 bases, the number alone and with at_set_edit_traceback
    one all-pairs overlap with at_set_min_score
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligntools.c_amd as A

LOCAL_LENS = [1, 2, 15, 16, 17, 40, 41, 48, 49, 56, 57, 63, 64, 65, 80, 81, 96, 104, 105, 112, 113, 128, 129, 150, 152, 160, 161, 207, 208,
              209, 250, 256, 257, 300, 304]
GLOBAL_LENS = [1, 2, 39, 40, 41, 48, 49, 56, 57, 64, 65, 80, 81, 104, 105, 128, 129, 150, 151, 152, 153, 160, 161, 200, 208, 209, 250, 256, 257, 300, 304]
LONG_LENS = [150, 300, 304, 305, 306, 319, 320, 321, 383, 384, 385, 415, 416, 417, 500, 511, 512, 513, 600, 607, 608]
SCORINGS = {"bench": (2, -2, -5, -2, -10), "mild": (1, -1, -2, -1, -4)}
SITES = [20, 100, 250, 400]

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
al = A.Aligner(0)
lib = A.load_library()
p = lambda a: a.ctypes.data_as(C.c_void_p)
rng = np.random.default_rng(2609)


def emit(case, cfg):
    out.write(json.dumps({"case": case, "last_config": cfg}) + "\n")
    out.flush()


def run(case, mode, blob, len1, len2, tb=True):
    """one at_align_batch over sequences laid back to back in blob (s1 of pair k, then its s2)"""
    n = len(len1)
    tot = len1.astype(np.int64) + len2
    off1 = np.concatenate(([0], np.cumsum(tot[:-1]))).astype(np.int64)
    off2 = off1 + len1
    score, ei, ej, st, nops = (np.zeros(n, np.int32) for _ in range(5))
    ops = np.zeros(int(tot.sum()) + 64, np.uint8)
    rc = lib.at_align_batch(al._h, A.MODES[mode], n, p(blob), p(off1), p(len1), p(off2), p(len2), 1 if tb else 0, p(score), p(ei), p(ej), p(st),
                            p(ops), p(off1), p(nops))
    emit(case, al.last_config if rc == 0 else "error %d: %s" % (rc, lib.at_last_error(al._h).decode()))
    if rc:   # (nothing more on a device that may have faulted)
        sys.exit(1)


def bases(n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), np.uint8)[rng.integers(0, len(alphabet), n)]


MODES = [("local", "local", False), ("global", "global", False), ("fit", "fit", False), ("fit -s", "fit", True), ("overlap", "overlap", False),
         ("edit", "edit", False)]

# ---- uniform ----
for l in (150, 1024):
    blob_all = bases(20000 * 2 * l)
    for n in (20000, 600):
        len1 = np.full(n, l, np.int32)
        for sname, sc in SCORINGS.items():
            for name, mode, uj in MODES:
                al.set_scoring(*sc, uj, SITES)
                run("uniform %dx%d %s n=%d scoring=%s" % (l, l, name, n, sname), mode, blob_all[:n * 2 * l], len1, len1)

# ---- ragged ----
for lname, lens in (("local list", LOCAL_LENS), ("global list", GLOBAL_LENS), ("long list", LONG_LENS)):
    n = 1400
    len1 = np.where(np.arange(n) % 4 > 0, rng.choice(lens, n), rng.integers(1, max(lens) + 1, n)).astype(np.int32)
    spread = rng.choice([0, 5, 60, 300], n)
    for alpha in ("ACGT", "ACGTN"):
        for name, mode, uj in MODES[:5]:
            # fit: l1 <= l2; the others: second sequences on both sides of the read's length
            len2 = (np.maximum(len1, 2) + spread if mode == "fit" else np.maximum(1, len1 - 40 + spread // 2)).astype(np.int32)
            blob = bases(int((len1.astype(np.int64) + len2).sum()) + 1, alpha)
            al.set_scoring(*SCORINGS["mild"], uj, SITES)
            for tb in ((True,) if mode == "overlap" else (True, False)):
                run("ragged %s %s %s tb=%d" % (lname, name, alpha, tb), mode, blob, len1, len2, tb)

# ---- edit ----
al.set_scoring(0, 1, 0, 0, 0, False, [])
for l in (64, 160, 1000):
    for n in (2000, 20000):
        len1 = np.full(n, l, np.int32)
        blob = bases(n * 2 * l)
        for etb in (False, True):
            al.set_edit_traceback(etb)
            run("edit %dx%d n=%d alignments=%d" % (l, l, n, etb), "edit", blob, len1, len1)
    lr = rng.integers(max(1, l // 2), l + 1, 2000).astype(np.int32)
    run("edit ragged ..%d n=2000 alignments=1" % l, "edit", bases(int(lr.sum()) * 2 + 1), lr, lr)
al.set_edit_traceback(False)

# ---- all-pairs overlap with a threshold ----
for l in (100, 300, 1000):
    nreads = 300
    lens = rng.integers(l // 2, l + 1, nreads).astype(np.int32)
    off = np.concatenate(([0], np.cumsum(lens[:-1]))).astype(np.int64)
    blob = bases(int(lens.sum()) + 1)
    al.set_scoring(1, -2, -5, -1, -10, False, [])
    for T in (None, 20):
        al.set_min_score(T)
        al.align_allpairs_stream("overlap", blob, off, lens, 0, nreads * (nreads - 1) // 2, 20000, lambda *a: None)
        emit("all-pairs overlap %d reads of ..%d min_score=%s" % (nreads, l, T), al.last_config)
    al.set_min_score(None)
al.close()
