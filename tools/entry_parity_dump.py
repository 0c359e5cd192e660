"""Every output array and at_last_config of the query-vs-target entries and at_allpairs_hits on a tiny fixed input, one JSON line
per call, to compare two builds of the library byte by byte (`AT_LIB_PATH=... entry_parity_dump.py OUT.jsonl`, then `cmp`):

    search in five modes, scan, scan_local and scan_hits on 6 queries of two lengths against 3 targets of 40, 173 and 400 bases,
    both strands; allpairs_hits in four modes on the 9 sequences; scans and allpairs_hits with CIGARs;
    the tiled scans (scan_local, scan_fit) once more where their tiles, blocks and windows differ: scan_fit with a fourth target of
    30 bases (shorter than the 37-base queries: the block filter and the length sort); both at tile_cols 16 and 64 (dropped tiles, a
    full and a ragged pass on the long targets, ragged-only short ones); both with min_score at half the perfect score of the 24-base
    queries; both with an N in one target (byte words) at tile_cols 16;
    all of it with AT_ALLPAIRS_CHUNK=7 (many slices) and unset

The millisecond figures in at_last_config (`sweep=`, `select=`) are blanked.  Seconds."""
import json
import os
import random
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aligntools.c_amd as A

UNIT = (1, 1, -5, -1, -10)
AFFINE = (2, -2, -5, -2, -10)

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
rng = random.Random(1818)
targets = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (40, 173, 400)]
queries = []
for q in range(6):
    t = targets[1 + q % 2]
    n = 24 if q < 3 else 37
    at = rng.randint(0, len(t) - n)
    s = "".join(rng.choice("ACGT") if rng.random() < 0.06 else c for c in t[at:at + n])
    queries.append(A.revcomp(s).decode() if q % 3 == 2 else s)
rng4 = random.Random(2121)
targets4 = targets + ["".join(rng4.choice("ACGT") for _ in range(30))]
targets_n = [targets[0], targets[1][:90] + "N" + targets[1][91:], targets[2], targets4[3]]


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        return {k: plain(x) for k, x in sorted(v.items())}
    return int(v) if isinstance(v, np.integer) else v


def emit(case, res, cfg):
    cfg = re.sub(r"(sweep|select)=[0-9.]+ms", r"\1=*ms", cfg)
    out.write(json.dumps({"case": case, "last_config": cfg, "results": plain(res)}, sort_keys=True) + "\n")
    out.flush()


al = A.Aligner(0)
for chunk in ("7", None):
    if chunk:
        os.environ["AT_ALLPAIRS_CHUNK"] = chunk
    else:
        os.environ.pop("AT_ALLPAIRS_CHUNK", None)
    tag = "chunk=%s " % chunk
    for mode in ("local", "global", "fit", "overlap", "edit"):
        al.set_scoring(*(UNIT if mode == "edit" else AFFINE))
        emit(tag + "search " + mode, al.search(mode, queries, targets, k=2, strands="both"), al.last_config)
    al.set_scoring(*UNIT)
    emit(tag + "scan", al.scan(queries, targets, k=2, strands="both", cigar=True), al.last_config)
    emit(tag + "scan cutoff", al.scan(queries, targets, k=3, cutoff=6, strands="both", cigar=True, cigar_m=True), al.last_config)
    emit(tag + "scan_hits", al.scan_hits(queries, targets, 5, strands="both", cigar=True), al.last_config)
    al.set_scoring(*AFFINE)
    emit(tag + "scan_local", al.scan_local(queries, targets, k=2, strands="both", cigar=True), al.last_config)
    reads = queries + targets
    for mode, threshold in (("overlap", 12), ("local", 30), ("global", -60), ("edit", 30)):
        al.set_scoring(*(UNIT if mode == "edit" else AFFINE))
        emit(tag + "allpairs_hits " + mode, al.allpairs_hits(mode, reads, threshold, cigar=mode != "edit"), al.last_config)
    al.set_scoring(*AFFINE)
    emit(tag + "scan_fit 4 targets", al.scan_fit(queries, targets4, k=2, strands="both", cigar=True), al.last_config)
    for tile in (16, 64):
        emit(tag + "scan_local tile=%d" % tile, al.scan_local(queries, targets4, k=2, strands="both", cigar=True, tile_cols=tile), al.last_config)
        emit(tag + "scan_fit tile=%d" % tile, al.scan_fit(queries, targets4, k=2, strands="both", cigar=True, tile_cols=tile), al.last_config)
    half = AFFINE[0] * 24 // 2
    emit(tag + "scan_local min_score", al.scan_local(queries, targets4, k=2, min_score=half, strands="both", cigar=True), al.last_config)
    emit(tag + "scan_fit min_score", al.scan_fit(queries, targets4, k=2, min_score=half, strands="both", cigar=True), al.last_config)
    emit(tag + "scan_local N", al.scan_local(queries, targets_n, k=2, strands="both", cigar=True, tile_cols=16), al.last_config)
    emit(tag + "scan_fit N", al.scan_fit(queries, targets_n, k=2, strands="both", cigar=True, tile_cols=16), al.last_config)
al.close()
