#!/usr/bin/env python3
"""search_rate.py -- rates of the query-vs-target search (at_search) on one GPU; one JSON line per measurement.

    python3 tools/search_rate.py [--cases abcs] [--reps 3] [--out FILE] [--parent-lib LIB]

  a  local 150 x 150, 20 000 queries x 500 targets (10 M pairs, k = 1): at_search end to end (host sequences in, nq x k hits
     out) against at_align_batch_device on the same 10 M pairs as one uniform device-resident batch, scores only -- the two
     alternate, `reps` times each; GCUPS = 10 M * 150 * 150 cells / seconds
  b  fit -s, 10 000 reads of 150 x 200 windows of 500 (k = 1)
  c  `alignTools batch local --queries q.fa t.fa` against `batch local --score-only` on the equivalent pair file (1 000 x 200):
     wall clock and output bytes
  s  both strands, the shape of case a (20 000 queries x 500 targets, k = 1: 20 M pairs): at_search_strands(BOTH) against what a
     caller had to do before it existed -- reverse-complement every query on the host, at_search on the 40 000 queries, merge the
     two hit lists per query -- with that at_search taken from --parent-lib (a build of the commit before at_search_strands; the
     same library when the option is absent).  The two alternate, `reps` times each after a warm-up; the host's time for the
     reverse complements and for the merge is reported separately.  `--cases S`: the both-strand search alone (for a kernel trace)
Kernel shares: run case a (or S) alone under `rocprofv3 --kernel-trace --stats` (tools/README.md).
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aligntools.c_amd as A  # noqa: E402

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def reads(rng, n, length):
    codes = rng.integers(0, 4, size=(n, length), dtype=np.uint8)
    return codes, [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[c]) for c in codes]


class Search:
    """at_search through ctypes with the host arrays built once (what a caller holding its sequences pays per call)."""

    def __init__(self, al, queries, targets):
        self.al = al

        def pack(seqs):
            lens = np.array([len(s) for s in seqs], dtype=np.int32)
            off = np.zeros(len(seqs), dtype=np.int64)
            off[1:] = np.cumsum(lens[:-1])
            return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy(), off, lens
        self.q, self.t = pack(queries), pack(targets)
        self.nq, self.nt = len(queries), len(targets)

    def run(self, mode, k=1):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        outs = [np.zeros(self.nq * k, dtype=np.int32) for _ in range(5)] + [np.zeros(self.nq, dtype=np.int32)]
        t0 = time.perf_counter()
        self.al._check(self.al._lib.at_search(self.al._h, mode, self.nq, p(self.q[0]), p(self.q[1]), p(self.q[2]), self.nt, p(self.t[0]),
                                              p(self.t[1]), p(self.t[2]), k, 0, 0, *[p(o) for o in outs]))
        return time.perf_counter() - t0, outs


def case_a(al, reps, out):
    import torch
    rng = np.random.default_rng(1)
    nq, nt, L = 20000, 500, 150
    qc, qs = reads(rng, nq, L)
    tc, ts = reads(rng, nt, L)
    al.set_scoring(1, -2, -5, -1, -10)
    s = Search(al, qs, ts)
    # the same pairs as one device-resident uniform batch: the read set packed 2 bits per base, 10 words + 1 slack word per read
    allc = np.concatenate([qc, tc]).astype(np.uint32)
    w = np.zeros((nq + nt, 11), dtype=np.uint32)
    for b in range(L):
        w[:, b // 16] |= allc[:, b] << np.uint32(2 * (b % 16))
    dev = torch.device("cuda", 0)
    d_words = torch.from_numpy(w.reshape(-1).view(np.int32)).to(dev)
    n = nq * nt
    d_woff1 = (torch.arange(nq, device=dev, dtype=torch.int64) * 11).repeat_interleave(nt)
    d_woff2 = ((torch.arange(nt, device=dev, dtype=torch.int64) + nq) * 11).repeat(nq)
    d_len = torch.full((n,), L, dtype=torch.int32, device=dev)
    d_res = torch.zeros((4, n), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def dev_batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        al.align_batch_device(A.MODE_LOCAL, n, d_words.data_ptr(), 2, d_woff1.data_ptr(), d_len.data_ptr(), d_woff2.data_ptr(), d_len.data_ptr(),
                              L, L, True, False, d_res[0].data_ptr(), d_res[1].data_ptr(), d_res[2].data_ptr(), d_res[3].data_ptr(), 0, 0, 0, stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    cells = float(n) * L * L
    dev_batch()
    s.run(A.MODE_LOCAL)                                                     # warm-up of both
    ts_search, ts_dev = [], []
    for _ in range(reps):
        ts_dev.append(dev_batch())
        dev_cfg = al.last_config
        dt, outs = s.run(A.MODE_LOCAL)
        ts_search.append(dt)
    # the search's hits against the device batch's scores (k = 1: the best target of every query, ties to the smaller index)
    sc = d_res[0].view(nq, nt).cpu().numpy()
    best = np.argmax(sc, axis=1)
    assert (outs[0] == best).all() and (outs[1] == sc[np.arange(nq), best]).all(), "search hits differ from the device batch"
    gs, gd = cells / min(ts_search) / 1e9, cells / min(ts_dev) / 1e9
    emit(out, dict(case="a", what="local 150x150, 20000 queries x 500 targets, k=1", pairs=n, reps=reps,
                   search_s=[round(x, 4) for x in ts_search], device_batch_s=[round(x, 4) for x in ts_dev],
                   search_gcups=round(gs, 1), device_batch_gcups=round(gd, 1), ratio=round(gs / gd, 3),
                   search_config=al.last_config, device_batch_config=dev_cfg))


COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


class ParentSearch(Search):
    """at_search of another build of the library (its own handle), loaded beside this one."""

    class _Al:
        pass

    def __init__(self, path, queries, targets):
        lib = C.CDLL(path)
        lib.at_init.restype = C.c_int
        lib.at_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        lib.at_last_error.restype = C.c_char_p
        lib.at_last_error.argtypes = [C.c_void_p]
        lib.at_last_config.restype = C.c_char_p
        lib.at_last_config.argtypes = [C.c_void_p]
        lib.at_set_scoring.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_int]
        lib.at_search.restype = C.c_int
        lib.at_search.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int, C.c_int32] + [C.c_void_p] * 6
        h = C.c_void_p()
        dev = (C.c_int * 1)(0)
        assert lib.at_init(dev, 1, C.byref(h)) == 0, lib.at_last_error(None)
        assert lib.at_set_scoring(h, 1, -2, -5, -1, -10, 0, (C.c_int * 1)(0), 0) == 0
        al = self._Al()
        al._lib, al._h = lib, h

        def check(rc):
            assert rc == 0, lib.at_last_error(h)
        al._check = check
        self.lib = lib
        super().__init__(al, queries, targets)


def strands_run(s, mode, k=1):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = [np.zeros(s.nq * k, dtype=np.int32) for _ in range(6)] + [np.zeros(s.nq, dtype=np.int32)]
    t0 = time.perf_counter()
    s.al._check(s.al._lib.at_search_strands(s.al._h, mode, s.nq, p(s.q[0]), p(s.q[1]), p(s.q[2]), s.nt, p(s.t[0]), p(s.t[1]), p(s.t[2]),
                                            k, 0, 0, A.STRAND_BOTH, *[p(o) for o in outs]))
    return time.perf_counter() - t0, outs


def case_s(al, reps, out, parent_lib, alone=False):
    rng = np.random.default_rng(4)
    nq, nt, L = 20000, 500, 150
    _, qs = reads(rng, nq, L)
    _, ts = reads(rng, nt, L)
    for t in range(0, nt, 2):                                               # half of the targets hold a stretch of a query, every
        q = qs[int(rng.integers(nq))]                                       # second one of its reverse complement
        if t & 2:
            q = q.translate(COMPLEMENT)[::-1]
        ts[t] = ts[t][:40] + q[40:120] + ts[t][120:]
    al.set_scoring(1, -2, -5, -1, -10)
    both = Search(al, qs, ts)
    cells = 2.0 * nq * nt * L * L
    if alone:
        strands_run(both, A.MODE_LOCAL)
        times = [strands_run(both, A.MODE_LOCAL)[0] for _ in range(reps)]
        emit(out, dict(case="S", what="local 150x150, 20000 queries x 500 targets, both strands, k=1", pairs=2 * nq * nt, reps=reps,
                       strands_s=[round(x, 4) for x in times], strands_gcups=round(cells / min(times) / 1e9, 1), strands_config=al.last_config))
        return

    def by_hand(first=False):
        """What a caller does without at_search_strands.  The first call also builds the parent's handle and arrays."""
        t0 = time.perf_counter()
        rc = [q.translate(COMPLEMENT)[::-1] for q in qs]
        t_rc = time.perf_counter() - t0
        if first:
            by_hand.s = ParentSearch(parent_lib, qs + rc, ts) if parent_lib else Search(al, qs + rc, ts)
        t_search, o = by_hand.s.run(A.MODE_LOCAL)                           # (its host arrays were built once, as `both`'s)
        t0 = time.perf_counter()
        f, r = slice(0, nq), slice(nq, 2 * nq)
        take_r = o[1][r] > o[1][f]                                          # ties: target index, then the query as given
        take_r |= (o[1][r] == o[1][f]) & (o[0][r] < o[0][f])
        merged = [np.where(take_r, x[r], x[f]) for x in o[:5]] + [take_r.astype(np.int32)]
        t_merge = time.perf_counter() - t0
        return t_rc, t_search, t_merge, merged
    by_hand(first=True)
    strands_run(both, A.MODE_LOCAL)                                         # warm-up of both
    ta, tb = [], []
    for _ in range(reps):
        tb.append(by_hand()[:3])
        dt, outs = strands_run(both, A.MODE_LOCAL)
        ta.append(dt)
    merged = by_hand()[3]
    for name, x, y in zip(("target", "score", "end_i", "end_j", "state", "strand"), outs, merged):
        assert (x == y).all(), "both-strand search differs from the merged one-strand searches in " + name
    e2e = [sum(x) for x in tb]
    emit(out, dict(case="s", what="local 150x150, 20000 queries x 500 targets, both strands, k=1", pairs=2 * nq * nt, reps=reps,
                   parent_lib=os.path.basename(parent_lib) if parent_lib else None,
                   strands_s=[round(x, 4) for x in ta],
                   by_hand_s=[round(x, 4) for x in e2e], by_hand_revcomp_s=[round(x[0], 4) for x in tb],
                   by_hand_search_s=[round(x[1], 4) for x in tb], by_hand_merge_s=[round(x[2], 4) for x in tb],
                   strands_gcups=round(cells / min(ta) / 1e9, 1), by_hand_gcups=round(cells / min(e2e) / 1e9, 1),
                   by_hand_search_gcups=round(cells / min(x[1] for x in tb) / 1e9, 1),
                   strand1_hits=int(outs[5].sum()), strands_config=al.last_config))


def case_b(al, reps, out):
    rng = np.random.default_rng(2)
    _, qs = reads(rng, 10000, 150)
    _, ts = reads(rng, 200, 500)
    al.set_scoring(1, -2, -5, -1, -10, True, list(range(20, 500, 37)))
    s = Search(al, qs, ts)
    s.run(A.MODE_FIT)
    times = [s.run(A.MODE_FIT)[0] for _ in range(reps)]
    cells = 10000.0 * 200 * 150 * 500
    emit(out, dict(case="b", what="fit -s, 10000 reads of 150 x 200 windows of 500, k=1", pairs=2000000, reps=reps,
                   search_s=[round(x, 4) for x in times], search_gcups=round(cells / min(times) / 1e9, 1), search_config=al.last_config))


def case_c(reps, out):
    rng = random.Random(3)
    nq, nt = 1000, 200
    qs = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(nq)]
    ts = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(nt)]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "q.fa"), "w") as fh:
            fh.writelines(">q%d\n%s\n" % (k, s) for k, s in enumerate(qs))
        with open(os.path.join(d, "t.fa"), "w") as fh:
            fh.writelines(">t%d\n%s\n" % (k, s) for k, s in enumerate(ts))
        with open(os.path.join(d, "pairs.fa"), "w") as fh:
            for a in range(nq):
                fh.writelines(">q%d\n%s\n>t%d\n%s\n" % (a, qs[a], b, ts[b]) for b in range(nt))
        runs = {"search": [EXE, "batch", "local", "--queries", "q.fa", "t.fa"],
                "search_score_only": [EXE, "batch", "local", "--queries", "q.fa", "--score-only", "t.fa"],
                "pair_file_score_only": [EXE, "batch", "local", "--score-only", "pairs.fa"]}
        rec = dict(case="c", what="alignTools batch local: --queries (1000 x 200) against --score-only on the pair file", pairs=nq * nt,
                   pair_file_bytes=os.path.getsize(os.path.join(d, "pairs.fa")))
        for _ in range(reps):
            for name, argv in runs.items():
                t0 = time.perf_counter()
                p = subprocess.run(argv, cwd=d, capture_output=True, timeout=300)
                dt = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr[-2000:]
                rec.setdefault(name + "_s", []).append(round(dt, 3))
                rec[name + "_out_bytes"] = len(p.stdout)
        emit(out, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="case s: a libaligntools_hip.so of the commit before at_search_strands")
    a = ap.parse_args()
    al = A.Aligner(0) if set(a.cases) & set("abSs") else None
    if "a" in a.cases:
        case_a(al, a.reps, a.out)
    if "b" in a.cases:
        case_b(al, a.reps, a.out)
    if "c" in a.cases:
        case_c(a.reps, a.out)
    if "s" in a.cases:
        case_s(al, a.reps, a.out, a.parent_lib)
    if "S" in a.cases:
        case_s(al, a.reps, a.out, None, alone=True)


if __name__ == "__main__":
    main()
