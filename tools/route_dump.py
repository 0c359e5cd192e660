"""Which kernel family, group width, rows per lane and storage class a fixed list of small batches takes: one JSON line per case
with at_last_config and a checksum of the batch's results (score, end_i, end_j, state, nops and the op bytes in use), to compare two
builds of the library on one card (`AT_LIB_PATH=... route_dump.py OUT.jsonl`; grids depend on the card): identical dumps are
identical routing AND identical outputs.  Under a minute:

    uniform 150 x 150 and 1024 x 1024 in every mode (fit also with -s), 20 000 and 600 pairs, two scorings, with tracebacks
    ragged: the read lengths around every row-class edge (the lists of tests/test_gpu_parity.py: local, global / fit, long reads),
            1 400 pairs each, local / global / fit / fit -s / overlap with tracebacks, ACGT and ACGT + N
    edit at 64 / 160 / 1 000 bases, the number alone and with at_set_edit_traceback
    edit infix (at_set_edit_infix) at 64 / 1 000 bases, the number alone and with the op lists
    one all-pairs overlap with at_set_min_score
    the device entry without the uniform promise, 4 096 pairs of 150 x 150 (the device decides: "auto: [...]")
    150 x 150 and 620 x 660 with tracebacks under the routing knobs of the packed path, one setting at a time
(No batch here has more work items than resident waves: the last round's sliver as 32-lane items is tests/test_knobs.py's.)
"""
import ctypes as C
import json
import os
import sys
import zlib

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


def emit(case, cfg, crc):
    out.write(json.dumps({"case": case, "last_config": cfg, "results_crc32": "%08x" % crc}) + "\n")
    out.flush()


def checksum(arrays, ops=None, ops_off=None, nops=None):
    """CRC-32 over the result arrays and, of the op buffer, the bytes each pair's list uses"""
    crc = 0
    for a in arrays:
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    if ops is not None:
        cnt = np.maximum(nops, 0).astype(np.int64)
        start = np.cumsum(cnt) - cnt
        idx = np.repeat(ops_off - start, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
        crc = zlib.crc32(ops[idx].tobytes(), crc)
    return crc


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
    emit(case, al.last_config if rc == 0 else "error %d: %s" % (rc, lib.at_last_error(al._h).decode()),
         checksum((score, ei, ej, st, nops), ops, off1, nops))
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

# ---- edit infix: reads inside targets three times their length ----
al.set_edit_infix(True)
for l in (64, 1000):
    n = 2000
    len1, len2 = np.full(n, l, np.int32), np.full(n, 3 * l, np.int32)
    blob = bases(n * 4 * l)
    for etb in (False, True):
        al.set_edit_traceback(etb)
        run("edit infix %dx%d n=%d alignments=%d" % (l, 3 * l, n, etb), "edit", blob, len1, len2)
al.set_edit_traceback(False)
al.set_edit_infix(False)

# ---- all-pairs overlap with a threshold ----
for l in (100, 300, 1000):
    nreads = 300
    lens = rng.integers(l // 2, l + 1, nreads).astype(np.int32)
    off = np.concatenate(([0], np.cumsum(lens[:-1]))).astype(np.int64)
    blob = bases(int(lens.sum()) + 1)
    al.set_scoring(1, -2, -5, -1, -10, False, [])
    for T in (None, 20):
        al.set_min_score(T)
        crc = [0]

        def on_slice(first, *arrays):
            crc[0] = checksum(arrays) ^ zlib.crc32(b"%d" % first, crc[0])
        al.align_allpairs_stream("overlap", blob, off, lens, 0, nreads * (nreads - 1) // 2, 20000, on_slice)
        emit("all-pairs overlap %d reads of ..%d min_score=%s" % (nreads, l, T), al.last_config, crc[0])
    al.set_min_score(None)

# ---- the device entry without the uniform promise ----
import torch

dev = torch.device("cuda", 0)


def run_device(case, mode, n, l1, l2, uniform):
    seqs = bases(n * (l1 + l2)).tobytes()
    pairs = [(seqs[k * (l1 + l2):k * (l1 + l2) + l1], seqs[k * (l1 + l2) + l1:(k + 1) * (l1 + l2)]) for k in range(n)]
    words, woff1, woff2, len1, len2, bits = A.pack_pairs(pairs)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("w", words.view(np.int32)), ("o1", woff1), ("o2", woff2), ("l1", len1), ("l2", len2))}
    res = torch.zeros((5, n), dtype=torch.int32, device=dev)
    ops = torch.zeros(n * (l1 + l2) + 64, dtype=torch.uint8, device=dev)
    ops_off = torch.arange(n, dtype=torch.int64, device=dev) * (l1 + l2)
    al.align_batch_device(A.MODES[mode], n, d["w"].data_ptr(), bits, d["o1"].data_ptr(), d["l1"].data_ptr(), d["o2"].data_ptr(), d["l2"].data_ptr(),
                          l1, l2, uniform, True, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), ops.data_ptr(),
                          ops_off.data_ptr(), res[4].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = res.cpu().numpy()
    emit(case, al.last_config, checksum(tuple(o), ops.cpu().numpy(), ops_off.cpu().numpy(), o[4]))


for name, mode, uj in MODES[:4]:
    al.set_scoring(*SCORINGS["bench"], uj, SITES)
    run_device("device entry, no uniform promise, 150x150 %s n=4096" % name, mode, 4096, 150, 150, False)

# ---- the packed path's routing knobs, one setting at a time ----
KNOBS = [{"AT_TWO_PASS": "2", "AT_TP_SPLIT": "0"}, {"AT_TWO_PASS": "2", "AT_TP_SPLIT": "1"}, {"AT_WALK_TEAMS": "0"}, {"AT_TAIL_SPLIT": "0"},
         {"AT_CK_PIECE_PAIRS": "96"}, {"AT_TP_RESERVE": "2"}]
for l1, l2 in ((150, 150), (620, 660)):
    n = 20000
    len1, len2 = np.full(n, l1, np.int32), np.full(n, l2, np.int32)
    blob = bases(n * (l1 + l2))
    for knobs in KNOBS:
        os.environ.update(knobs)
        for name, mode, uj in MODES[:4]:
            al.set_scoring(*SCORINGS["bench"], uj, SITES)
            run("knobs %s: uniform %dx%d %s n=%d" % (" ".join("%s=%s" % kv for kv in sorted(knobs.items())), l1, l2, name, n), mode, blob, len1, len2)
        for k in knobs:
            del os.environ[k]
al.close()
