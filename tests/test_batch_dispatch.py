"""The batch dispatch (align_device) seen from the public entries.

Settings survive the entries: at_scan's window pass is an infix batch with op lists and at_allpairs_hits' overlap slices run the
bit-parallel bound with the call's threshold, whatever the handle's settings say.  Those are settings of the CALL: the handle's own
(at_set_edit_infix, at_set_edit_traceback, at_set_min_score) are the same afterwards, whether the entry succeeds or is refused.
The refused cases (a 1 025-base query, edit with CIGARs) are refusals of the ENTRY, taken before it makes a request: they show that
a refused call leaves the settings alone, not what a failure below align_device leaves behind.

Refusal texts: every refusal of the batch dispatch that a public entry can reach, with its return code and the whole text of
at_last_error, through the device entries.  Each returns before a launch: the device pointers are never followed."""
import ctypes as C
import random

import numpy as np
import pytest

import aligntools.c_amd as A
import oracle as O

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_RANGE, ERR_DOMAIN = -1, -3, -4
UNIT = (1, 1, -5, -1, -10)        # u = 1: at_scan and the bit-parallel edit distance
OVERLAP = (1, -2, -5, -1, -10)    # a scoring the overlap filter applies to (m >= 0, 2 c > m)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s, rate=0.05):
    return "".join(rng.choice("ACGT") if rng.random() < rate else c for c in s)


def _scan_inputs():
    """6 queries of two lengths cut from 3 targets of 40, 173 and 400 bases"""
    rng = random.Random(1717)
    targets = [_rand(rng, n) for n in (40, 173, 400)]
    queries = []
    for q in range(6):
        t = targets[1 + q % 2]
        n = 24 if q < 3 else 37
        at = rng.randint(0, len(t) - n)
        s = _mutate(rng, t[at:at + n])
        queries.append(A.revcomp(s).decode() if q % 3 == 2 else s)
    return queries, targets


def _edit_pairs():
    rng = random.Random(1718)
    pairs = []
    for n in (1, 17, 64, 65, 150):
        s1 = _rand(rng, n)
        pairs.append((s1, _mutate(rng, s1, 0.1) + _rand(rng, rng.randint(0, 9))))
    return pairs


def _edit_batch_with_traceback(al, pairs):
    """at_align_batch in edit mode with want_traceback and op buffers (Aligner.align_batch asks for no traceback while its own copy
    of the setting is off): (scores, at_last_config)"""
    enc = [(a.encode(), b.encode()) for a, b in pairs]
    n = len(enc)
    len1 = np.array([len(a) for a, _ in enc], dtype=np.int32)
    len2 = np.array([len(b) for _, b in enc], dtype=np.int32)
    tot = len1.astype(np.int64) + len2
    off1 = np.concatenate(([0], np.cumsum(tot[:-1]))).astype(np.int64)
    off2 = off1 + len1
    blob = np.frombuffer(b"".join(a + b for a, b in enc) + b"\0", dtype=np.uint8).copy()
    score, ei, ej, st, nops = (np.full(n, -99, np.int32) for _ in range(5))
    ops = np.zeros(int(tot.sum()) + 64, np.uint8)
    rc = al._lib.at_align_batch(al._h, A.MODE_EDIT, n, _p(blob), _p(off1), _p(len1), _p(off2), _p(len2), 1, _p(score), _p(ei), _p(ej),
                                _p(st), _p(ops), _p(off1), _p(nops))
    assert rc == 0, al._lib.at_last_error(al._h)
    return score, al.last_config


def _allpairs_overlap(al, reads):
    """at_align_allpairs in overlap mode, scores only: ((4, pairs) results, at_last_config)"""
    enc = [r.encode() for r in reads]
    lens = np.array([len(r) for r in enc], dtype=np.int32)
    off = np.zeros(len(enc), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    blob = np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8).copy()
    npairs = len(enc) * (len(enc) - 1) // 2
    out = [np.full(npairs, -99, dtype=np.int32) for _ in range(4)]
    rc = al._lib.at_align_allpairs(al._h, A.MODE_OVERLAP, len(enc), _p(blob), _p(off), _p(lens), 0, npairs, 0, _p(out[0]), _p(out[1]),
                                   _p(out[2]), _p(out[3]), None, None, None)
    assert rc == 0, al._lib.at_last_error(al._h)
    return np.array(out), al.last_config


def _overlap_reads():
    """8 reads of 50-90 bases cut at overlapping offsets from one sequence: true dovetails and unrelated pairs"""
    rng = random.Random(1719)
    genome = _rand(rng, 260)
    reads = []
    for _ in range(8):
        n = rng.randint(50, 90)
        at = rng.randint(0, 260 - n)
        reads.append(_mutate(rng, genome[at:at + n], 0.03))
    return reads


@pytest.fixture(scope="module")
def handle():
    al = A.Aligner(0)
    yield al
    al.close()


@pytest.mark.parametrize("fail_between", (False, True))
def test_scan_leaves_the_edit_settings(handle, fail_between):
    al = handle
    al.set_scoring(*UNIT)
    al.set_edit_infix(False)
    al.set_edit_traceback(False)
    queries, targets = _scan_inputs()
    if fail_between:
        with pytest.raises(A.AlignToolsError) as ei:
            al.scan(["A" * 1025] + queries, targets, k=2, strands="both", cigar=True)
        assert (ei.value.code, al._lib.at_last_error(al._h).decode()) == (ERR_DOMAIN, "at_scan: query 0 has 1025 bases, more than 1024")
    else:
        res = al.scan(queries, targets, k=2, strands="both", cigar=True)
        assert (res["nhits"] > 0).all() and "windows: myers-infix-tb" in al.last_config, al.last_config
    pairs = _edit_pairs()
    score, cfg = _edit_batch_with_traceback(al, pairs)
    assert cfg.startswith("myers bits=2"), cfg
    want = [O.align(O.EDIT, a.encode(), b.encode(), *UNIT)["score"] for a, b in pairs]
    assert score.tolist() == want


@pytest.mark.parametrize("fail_between", (False, True))
def test_allpairs_hits_leaves_the_threshold(handle, fail_between):
    al = handle
    al.set_scoring(*OVERLAP)
    al.set_edit_infix(False)
    al.set_edit_traceback(False)
    al.set_min_score(None)
    reads = _overlap_reads()
    if fail_between:
        with pytest.raises(A.AlignToolsError) as ei:
            al.allpairs_hits("edit", reads, 10, cigar=True)
        assert (ei.value.code, al._lib.at_last_error(al._h).decode()) == (
            ERR_ARG, "at_allpairs_hits: edit has no CIGAR here (alignments of edit distances: at_align_batch_cigar)")
    else:
        hits = al.allpairs_hits("overlap", reads, 10)
        assert len(hits["pair"]) > 0 and "overlap filter" in al.last_config, al.last_config
    got, cfg = _allpairs_overlap(al, reads)
    assert "overlap filter" not in cfg, cfg
    enc = [r.encode() for r in reads]
    want = [[O.align(O.OVERLAP, enc[a], enc[b], *OVERLAP)[name] for a in range(len(enc)) for b in range(a + 1, len(enc))]
            for name in ("score", "end_i", "end_j", "state")]
    assert got.tolist() == want


# ---------------------------------------------------------------- refusal texts

BENCH = (2, -2, -5, -2, -10)
TWO = (0, 2, 0, 0, 0)             # u = 2: outside the bit-parallel edit paths
INFIX_LDS = "64 windows of packed words in 60 KB of LDS"

# (id, scoring, edit infix, edit alignments, entry, overrides of the valid call, code, text)
REFUSALS = [
    ("mode-high", BENCH, 0, 0, "batch", dict(mode=5), ERR_ARG, "unknown mode 5"),
    ("mode-negative", BENCH, 0, 0, "batch", dict(mode=-1), ERR_ARG, "unknown mode -1"),
    ("mode-allpairs", BENCH, 0, 0, "allpairs", dict(mode=9), ERR_ARG, "unknown mode 9"),
    ("npairs-negative", BENCH, 0, 0, "batch", dict(npairs=-1), ERR_ARG, "negative size"),
    ("max_len1-negative", BENCH, 0, 0, "batch", dict(max_len1=-1), ERR_ARG, "negative size"),
    ("max_len2-negative", BENCH, 0, 0, "batch", dict(max_len2=-1), ERR_ARG, "negative size"),
    ("bits-4", BENCH, 0, 0, "batch", dict(bits=4), ERR_ARG, "bits must be 2 or 8"),
    ("bits-0-allpairs", BENCH, 0, 0, "allpairs", dict(bits=0), ERR_ARG, "bits must be 2 or 8"),
    ("null-seq", BENCH, 0, 0, "batch", dict(d_seq=None), ERR_ARG, "NULL device pointer"),
    ("null-woff1", BENCH, 0, 0, "batch", dict(d_woff1=None), ERR_ARG, "NULL device pointer"),
    ("null-len1", BENCH, 0, 0, "batch", dict(d_len1=None), ERR_ARG, "NULL device pointer"),
    ("null-woff2", BENCH, 0, 0, "batch", dict(d_woff2=None), ERR_ARG, "NULL device pointer"),
    ("null-len2", BENCH, 0, 0, "batch", dict(d_len2=None), ERR_ARG, "NULL device pointer"),
    ("null-score", BENCH, 0, 0, "batch", dict(d_score=None), ERR_ARG, "NULL device pointer"),
    ("null-len-allpairs", BENCH, 0, 0, "allpairs", dict(d_len=None), ERR_ARG, "NULL device pointer"),
    ("null-ops", BENCH, 0, 0, "batch", dict(want_traceback=1, d_ops=None), ERR_ARG, "traceback wanted but ops buffers are NULL"),
    ("null-ops_off", BENCH, 0, 0, "batch", dict(want_traceback=1, d_ops_off=None), ERR_ARG, "traceback wanted but ops buffers are NULL"),
    ("null-nops", BENCH, 0, 0, "allpairs", dict(want_traceback=1, d_nops=None), ERR_ARG, "traceback wanted but ops buffers are NULL"),
    ("null-ops-edit", UNIT, 0, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1, d_nops=None), ERR_ARG,
     "traceback wanted but ops buffers are NULL"),
    ("null-ops-infix", UNIT, 1, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1, d_ops=None), ERR_ARG,
     "traceback wanted but ops buffers are NULL"),
    ("exact-range", BENCH, 0, 0, "batch", dict(max_len1=1 << 20, max_len2=1 << 20), ERR_RANGE,
     "scores may exceed the exact range: max|param|=10, l1+l2=2097152"),
    ("exact-range-edge", (8, -2, -5, -2, -1), 0, 0, "batch", dict(max_len1=1 << 20, max_len2=(1 << 20) - 2), ERR_RANGE,
     "scores may exceed the exact range: max|param|=8, l1+l2=2097150"),
    ("infix-allpairs", UNIT, 1, 0, "allpairs", dict(mode=A.MODE_EDIT), ERR_DOMAIN, "edit infix mode: no all-vs-all (pair lists and searches only)"),
    ("infix-u", TWO, 1, 0, "batch", dict(mode=A.MODE_EDIT), ERR_DOMAIN, "edit infix mode needs the unit mismatch cost: u = 2, not 1"),
    ("infix-bits", UNIT, 1, 0, "batch", dict(mode=A.MODE_EDIT, bits=8), ERR_DOMAIN,
     "edit infix mode needs a 2-bit batch: some base is not one of ACGT"),
    ("infix-len1", UNIT, 1, 1, "batch", dict(mode=A.MODE_EDIT, max_len1=1025), ERR_DOMAIN, "edit infix mode: max_len1 = 1025 exceeds 1024"),
    ("infix-len2", UNIT, 1, 0, "batch", dict(mode=A.MODE_EDIT, max_len2=3793), ERR_DOMAIN,
     "edit infix mode: max_len2 = 3793 exceeds 3792 (%s)" % INFIX_LDS),
    # (the first failing check decides: the cost before the alphabet, the alphabet before the lengths)
    ("infix-order", TWO, 1, 1, "batch", dict(mode=A.MODE_EDIT, bits=8, max_len1=1025, want_traceback=1), ERR_DOMAIN,
     "edit infix mode needs the unit mismatch cost: u = 2, not 1"),
    ("edit-tb-u", TWO, 0, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1), ERR_DOMAIN,
     "edit alignments need the unit mismatch cost: u = 2, not 1"),
    ("edit-tb-bits", UNIT, 0, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1, bits=8), ERR_DOMAIN,
     "edit alignments need a 2-bit batch: some base is not one of ACGT"),
    ("edit-tb-len1", UNIT, 0, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1, max_len1=1025), ERR_DOMAIN,
     "edit alignments: max_len1 = 1025 exceeds 1024"),
    ("edit-tb-len2", UNIT, 0, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1, max_len2=3793), ERR_DOMAIN,
     "edit alignments: max_len2 = 3793 exceeds 3792 (%s)" % INFIX_LDS),
    ("edit-tb-order", UNIT, 0, 1, "batch", dict(mode=A.MODE_EDIT, want_traceback=1, bits=8, max_len2=3793), ERR_DOMAIN,
     "edit alignments need a 2-bit batch: some base is not one of ACGT"),
    ("int32-2bit-scores", (8, -2, -5, -2, -10), 0, 0, "batch", dict(), ERR_RANGE,
     "the int32 2-bit kernels need |16*score| <= 127 (m=8 u=-2 o=-5): pack the batch with bits=8"),
    ("int32-2bit-scores-allpairs", (1, -8, -5, -1, -10), 0, 0, "allpairs", dict(mode=A.MODE_LOCAL), ERR_RANGE,
     "the int32 2-bit kernels need |16*score| <= 127 (m=1 u=-8 o=-5): pack the batch with bits=8"),
]

BATCH_ORDER = ["mode", "npairs", "d_seq", "bits", "d_woff1", "d_len1", "d_woff2", "d_len2", "max_len1", "max_len2", "uniform_shape",
               "want_traceback", "d_score", "d_end_i", "d_end_j", "d_state", "d_ops", "d_ops_off", "d_nops", "stream"]
ALLPAIRS_ORDER = ["mode", "nreads", "d_seq", "bits", "d_woff", "d_len", "max_len", "first_pair", "npairs", "want_traceback", "d_score",
                  "d_end_i", "d_end_j", "d_state", "d_ops", "d_ops_off", "d_nops", "stream"]


@pytest.fixture(scope="module")
def device_block():
    """a zeroed device buffer every pointer of a refused call points into (no refusal follows one)"""
    import torch
    return torch.zeros(4096, dtype=torch.int64, device="cuda:0")


def _device_call(al, entry, block, over):
    ptr = block.data_ptr()
    a = dict(mode=A.MODE_GLOBAL, npairs=4, nreads=4, first_pair=0, bits=2, max_len1=32, max_len2=32, max_len=32, uniform_shape=0, want_traceback=0,
             stream=None)
    a.update({name: ptr for name in BATCH_ORDER + ALLPAIRS_ORDER if name.startswith("d_")})
    a.update(over)
    fn, order = (al._lib.at_align_batch_device, BATCH_ORDER) if entry == "batch" else (al._lib.at_align_allpairs_device, ALLPAIRS_ORDER)
    rc = fn(al._h, *[a[name] for name in order])
    return rc, al._lib.at_last_error(al._h).decode()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal_text(handle, device_block, case):
    _, scoring, infix, edit_tb, entry, over, code, text = case
    al = handle
    al.set_scoring(*scoring)
    al.set_min_score(None)
    al.set_edit_infix(bool(infix))
    al.set_edit_traceback(bool(edit_tb))
    try:
        before = al.last_config
        assert _device_call(al, entry, device_block, over) == (code, text)
        assert al.last_config == before          # (a refusal is no launch: the configuration text stays)
    finally:
        al.set_edit_infix(False)
        al.set_edit_traceback(False)


def test_no_pairs_is_no_refusal(handle, device_block):
    """npairs == 0 returns AT_OK in front of the pointer checks"""
    al = handle
    al.set_scoring(*BENCH)
    nul = {name: None for name in BATCH_ORDER if name.startswith("d_") and name not in ("d_woff2", "d_len2")}
    assert _device_call(al, "batch", device_block, dict(npairs=0, **nul))[0] == 0
