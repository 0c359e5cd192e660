"""at_allpairs_hits / Aligner.allpairs_hits: all-vs-all of which only the pairs over a threshold leave the device.

The expected result everywhere is the dense existing entry -- align_allpairs_stream on a handle with no threshold set -- filtered
on the host: pair / a / b / score / end cell / state of the kept pairs, in ascending pair order.  The CIGARs of the hits are
compared with align_batch_cigar on the hit pairs."""
import ctypes as C
import random

import numpy as np
import pytest

import aligntools.c_amd as A

pytestmark = pytest.mark.gpu

MODES = ("overlap", "local", "global", "edit")
GUARD = -77


def _reads1():
    """48 reads of 60-220 bases cut at overlapping offsets from a 1 500-base sequence, about 3 % substitutions: dozens of true
    dovetails; two identical reads and a read of length 1"""
    rng = random.Random(1301)
    genome = "".join(rng.choice("ACGT") for _ in range(1500))
    reads = []
    for _ in range(48):
        n = rng.randint(60, 220)
        at = rng.randint(0, 1500 - n)
        r = list(genome[at:at + n])
        for x in range(n):
            if rng.random() < 0.03:
                r[x] = rng.choice("ACGT".replace(r[x], ""))
        reads.append("".join(r))
    reads[10] = reads[9]
    reads[20] = "G"
    return reads


def _reads2():
    """set 1 with an N in three reads: the 8-bit path, on which the bound does not apply"""
    reads = _reads1()
    for k, at in ((3, 17), (25, 0), (40, 59)):
        reads[k] = reads[k][:at] + "N" + reads[k][at + 1:]
    return reads


def _reads3():
    """six reads of 1 030-1 100 bases, past the bound's 1 024: every pair is swept"""
    rng = random.Random(1303)
    genome = "".join(rng.choice("ACGT") for _ in range(1500))
    reads = []
    for _ in range(6):
        n = rng.randint(1030, 1100)
        at = rng.randint(0, 1500 - n)
        r = list(genome[at:at + n])
        for x in range(n):
            if rng.random() < 0.03:
                r[x] = rng.choice("ACGT".replace(r[x], ""))
        reads.append("".join(r))
    return reads


SETS = {"set1": _reads1, "set2-N": _reads2, "set3-long": _reads3}


def _flat(reads):
    rs = [r.encode() for r in reads]
    lens = np.array([len(r) for r in rs], dtype=np.int32)
    off = np.zeros(len(rs), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    return np.frombuffer(b"".join(rs) + b"\0", dtype=np.uint8).copy(), off, lens


def _tri(n):
    a, b = np.triu_indices(n, 1)
    return a.astype(np.int32), b.astype(np.int32)


def _dense_on(al, mode, reads, first=0, npairs=None):
    blob, off, lens = _flat(reads)
    n = len(reads)
    total = n * (n - 1) // 2
    npairs = total - first if npairs is None else npairs
    out = {k: np.zeros(npairs, dtype=np.int32) for k in ("score", "end_i", "end_j", "state")}

    def on_slice(p0, sc, ei, ej, st):
        lo = p0 - first
        for k, v in zip(("score", "end_i", "end_j", "state"), (sc, ei, ej, st)):
            out[k][lo:lo + len(v)] = v
    al.align_allpairs_stream(mode, blob, off, lens, first, npairs, 0, on_slice)
    return out


def _prep(al, mode):
    """the default scoring; edit with the unit mismatch cost (the bit-parallel kernel)"""
    al.set_scoring(1, 1 if mode == "edit" else -2, -5, -1)
    return al


_dense_cache = {}


def _dense(setname, mode):
    """the dense reference of a (set, mode), computed once on a fresh handle with no threshold, and left unchanged"""
    key = (setname, mode)
    if key not in _dense_cache:
        al = _prep(A.Aligner(), mode)
        d = _dense_on(al, mode, SETS[setname]())
        al.close()
        for v in d.values():
            v.setflags(write=False)
        _dense_cache[key] = d
    return _dense_cache[key]


def _kept(d, mode, T):
    return d["score"] <= T if mode == "edit" else d["score"] >= T


def _expect(d, mode, T, nreads, first=0, npairs=None):
    a, b = _tri(nreads)
    total = len(a)
    npairs = total - first if npairs is None else npairs
    sel = np.zeros(total, dtype=bool)
    sel[first:first + npairs] = True
    sel &= _kept(d, mode, T)
    idx = np.nonzero(sel)[0]
    return dict(pair=idx.astype(np.int64), a=a[idx], b=b[idx], score=d["score"][idx], end_i=d["end_i"][idx], end_j=d["end_j"][idx],
                state=d["state"][idx])


def _threshold_keeping(d, mode, about):
    """the threshold in between (>= 5 kept, >= 5 dropped) that keeps about `about` pairs"""
    total = len(d["score"])
    return min((int(x) for x in np.unique(d["score"]) if 5 <= int(_kept(d, mode, x).sum()) <= total - 5),
               key=lambda x: abs(int(_kept(d, mode, x).sum()) - about))


def _thresholds(d, mode):
    """below every score, above every score, and the two extreme thresholds in between that keep >= 5 and drop >= 5 pairs"""
    sc = d["score"]
    lo, hi = int(sc.min()) - 1, int(sc.max()) + 1
    mid = [int(T) for T in np.unique(sc) if 5 <= int(_kept(d, mode, T).sum()) <= len(sc) - 5]
    assert len(mid) >= 2, "the set has no two thresholds that keep at least 5 pairs and drop at least 5"
    everything, nothing = (hi, lo) if mode == "edit" else (lo, hi)
    return everything, nothing, mid[0], mid[-1]


def _same(got, want):
    for k in ("pair", "a", "b", "score", "end_i", "end_j", "state"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.all(np.diff(got["pair"]) > 0)


@pytest.fixture(scope="module")
def al():
    x = A.Aligner()
    yield x
    x.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("setname", list(SETS))
def test_hits_equal_the_filtered_dense_run(al, setname, mode):
    reads = SETS[setname]()
    d = _dense(setname, mode)
    _prep(al, mode)
    everything, nothing, t1, t2 = _thresholds(d, mode)
    total = len(d["score"])
    for T in (everything, nothing, t1, t2):
        want = _expect(d, mode, T, len(reads))
        if T == everything:
            assert len(want["pair"]) == total
        elif T == nothing:
            assert len(want["pair"]) == 0
        else:
            assert 5 <= len(want["pair"]) <= total - 5
        got = al.allpairs_hits(mode, reads, T)
        _same(got, want)
        cfg = al.last_config
        assert cfg.startswith("allpairs-hits: threshold=%d, " % T) and ("kept=%d; " % len(want["pair"])) in cfg, cfg
    if mode == "overlap":
        # the bound: engaged on 2-bit reads of up to 1 024 bases, every pair swept elsewhere
        al.allpairs_hits(mode, reads, t2)
        assert ("overlap filter" in al.last_config) == (setname == "set1"), al.last_config


@pytest.mark.parametrize("mode", MODES)
def test_slices_and_ranges(al, mode):
    reads = _reads1()
    n = len(reads)
    total = n * (n - 1) // 2
    d = _dense("set1", mode)
    _prep(al, mode)
    _, _, t1, _ = _thresholds(d, mode)
    t2 = _threshold_keeping(d, mode, total // 4)
    want = _expect(d, mode, t1, n)
    for chunk in (1, 7, 97, 0):
        _same(al.allpairs_hits(mode, reads, t1, chunk_pairs=chunk), want)
    # first_pair > 0 with npairs ending mid-row, an empty range, the last pair alone
    for first, npairs in ((n + 5, 3 * n + 11), (100, 0), (total - 1, 1), (0, 1)):
        for T in (t1, t2):
            got = al.allpairs_hits(mode, reads, T, first_pair=first, npairs=npairs, chunk_pairs=97)
            _same(got, _expect(d, mode, T, n, first, npairs))
    want = _expect(d, mode, t2, n, n + 5, 3 * n + 11)
    assert 0 < len(want["pair"]) < len(_expect(d, mode, t2, n)["pair"])


def _raw(al, mode, reads, T, hit_cap, cigar=False, cigar_cap=0, flags=0, nbuf=None, first=0, npairs=None):
    """the C entry with guard values in every output"""
    blob, off, lens = _flat(reads)
    n = len(reads)
    npairs = n * (n - 1) // 2 - first if npairs is None else npairs
    nbuf = hit_cap if nbuf is None else nbuf
    o = dict(pair=np.full(nbuf + 1, GUARD, dtype=np.int64))
    for k in ("a", "b", "score", "end_i", "end_j", "state"):
        o[k] = np.full(nbuf + 1, GUARD, dtype=np.int32)
    if cigar:
        o["stats"] = np.full((nbuf + 1, 8), GUARD, dtype=np.int32)
        o["ncigar"] = np.full(nbuf + 1, GUARD, dtype=np.int32)
        o["cigar_off"] = np.full(nbuf + 2, GUARD, dtype=np.int64)
        o["words"] = np.full(cigar_cap + 8, 0xdeadbeef, dtype=np.uint32)
    nhits = C.c_int64(GUARD)
    p = A._ptr
    rc = al._lib.at_allpairs_hits(al._h, A.MODES[mode], n, p(blob), p(off), p(lens), first, npairs, int(T), 0, flags, hit_cap,
                                  C.addressof(nhits), p(o["pair"]), p(o["a"]), p(o["b"]), p(o["score"]), p(o["end_i"]), p(o["end_j"]),
                                  p(o["state"]), p(o.get("stats")), p(o.get("ncigar")), p(o.get("cigar_off")), p(o.get("words")), cigar_cap)
    return rc, int(nhits.value), o


@pytest.mark.parametrize("mode", ("overlap", "edit"))
def test_capacity_protocol(al, mode):
    reads = _reads1()
    d = _dense("set1", mode)
    _prep(al, mode)
    _, _, t1, _ = _thresholds(d, mode)
    want = _expect(d, mode, t1, len(reads))
    k = len(want["pair"])
    cg = mode != "edit"
    rc, nh, o = _raw(al, mode, reads, t1, k - 1, cigar=cg, cigar_cap=64 * k)
    assert rc == 0 and nh == k
    for name, arr in o.items():
        guard = 0xdeadbeef if name == "words" else GUARD
        assert np.all(arr == guard), name
    rc, nh, o = _raw(al, mode, reads, t1, k, cigar=cg, cigar_cap=64 * k)
    assert rc == 0 and nh == k
    _same({x: o[x][:k] for x in ("pair", "a", "b", "score", "end_i", "end_j", "state")}, want)
    for name in ("pair", "a", "b", "score", "end_i", "end_j", "state"):
        assert o[name][k] == GUARD
    if cg:
        assert o["cigar_off"][0] == 0 and o["cigar_off"][k] == o["ncigar"][:k].sum() and o["cigar_off"][k + 1] == GUARD


@pytest.mark.parametrize("mode", ("overlap", "local", "global"))
@pytest.mark.parametrize("setname", ("set1", "set2-N"))
def test_cigars_equal_the_batch_entry(al, setname, mode):
    reads = SETS[setname]()
    d = _dense(setname, mode)
    _prep(al, mode)
    total = len(d["score"])
    T = _threshold_keeping(d, mode, 40)
    want = _expect(d, mode, T, len(reads))
    k = len(want["pair"])
    assert 5 <= k <= total - 5
    pairs = [(reads[a], reads[b]) for a, b in zip(want["a"], want["b"])]
    for m in (False, True):
        ref = al.align_batch_cigar(mode, pairs, extended=not m)
        got = al.allpairs_hits(mode, reads, T, cigar=True, cigar_m=m, chunk_pairs=97)
        _same(got, want)
        assert "; alignments: " in al.last_config
        assert np.array_equal(ref["score"], want["score"]) and np.array_equal(ref["end_i"], want["end_i"]) and np.array_equal(ref["end_j"], want["end_j"])
        assert np.array_equal(got["ncigar"], ref["ncigar"])
        assert np.array_equal(got["cigar_off"], ref["cigar_off"])
        assert np.array_equal(got["stats"], ref["stats"])
        assert len(got["cigar"]) == k
        for e in range(k):
            assert np.array_equal(got["cigar"][e], ref["cigar"][e]), e
        letters = {A.CIGAR_LETTERS[int(w) & 15] for c in got["cigar"] for w in c}
        assert (ord("M") in letters) == m and (ord("=") in letters) == (not m)


def test_cigar_cap_too_small(al):
    reads = _reads1()
    d = _dense("set1", "overlap")
    _prep(al, "overlap")
    t2 = _threshold_keeping(d, "overlap", 40)
    full = al.allpairs_hits("overlap", reads, t2, cigar=True)
    k = len(full["pair"])
    off = full["cigar_off"]
    assert k >= 5 and off[k] > off[3] > 0
    cap = int(off[3]) + 1 if off[4] > off[3] + 1 else int(off[3])      # room for the first three hits, not for the fourth
    assert off[3] <= cap < off[4]
    rc, nh, o = _raw(al, "overlap", reads, t2, k, cigar=True, cigar_cap=cap)
    assert rc == 0 and nh == k
    assert np.array_equal(o["cigar_off"][:k + 1], off) and np.array_equal(o["ncigar"][:k], full["ncigar"])
    assert np.array_equal(o["stats"][:k], full["stats"])
    assert np.array_equal(o["words"][:off[3]], np.concatenate(full["cigar"][:3]))
    assert np.all(o["words"][off[3]:] == 0xdeadbeef)


def test_edit_has_no_cigar_and_other_refusals(al):
    reads = _reads1()
    d = _dense("set1", "overlap")
    _, _, t1, _ = _thresholds(d, "overlap")
    _prep(al, "overlap")
    rc, _, _ = _raw(al, "edit", reads, 30, 16, cigar=True, cigar_cap=64)
    assert rc == A.ERR_ARG
    rc, _, _ = _raw(al, "fit", reads, 30, 16)
    assert rc == A.ERR_ARG
    rc, _, _ = _raw(al, "overlap", reads, t1, -1, nbuf=4)
    assert rc == A.ERR_ARG
    al.set_edit_infix(True)
    try:
        rc, _, _ = _raw(al, "edit", reads, 30, 16)
        assert rc == A.ERR_DOMAIN
    finally:
        al.set_edit_infix(False)
    # the handle works afterwards
    _same(al.allpairs_hits("overlap", reads, t1), _expect(d, "overlap", t1, len(reads)))
    with pytest.raises(A.AlignToolsError):
        al.allpairs_hits("edit", reads, 30, cigar=True)


def test_handle_keeps_its_min_score_setting():
    reads = _reads1()
    d = _dense("set1", "overlap")
    _, _, t1, t2 = _thresholds(d, "overlap")
    al = _prep(A.Aligner(), "overlap")
    al.allpairs_hits("overlap", reads, t2)
    after = _dense_on(al, "overlap", reads)
    assert np.all(after["state"] == 2)
    for k in after:
        assert np.array_equal(after[k], d[k]), k
    al.set_min_score(t1)
    al.allpairs_hits("overlap", reads, t2)
    kept = _dense_on(al, "overlap", reads)
    al.close()
    fresh = _prep(A.Aligner(), "overlap")
    fresh.set_min_score(t1)
    ref = _dense_on(fresh, "overlap", reads)
    fresh.close()
    assert (ref["state"] == 0).sum() > 0
    for k in kept:
        assert np.array_equal(kept[k], ref[k]), k


def _pair_in(text):
    import re
    m = re.search(r"pair (\d+)", text)
    return int(m.group(1)) if m else None


@pytest.mark.parametrize("mode", MODES)
def test_domain_and_range_errors_as_the_dense_entry(mode):
    """Scoring blocks on both sides of the shim's exact-range check (max |parameter| * (l1 + l2 + 2) < 2^24; 442 for set 1, so
    37 000 passes and 38 000 does not): whatever the dense entry returns on the set -- a result, or an error code and, in the text,
    a pair index -- this entry returns too.  (On the all-pairs path no scoring block reaches a pair with score INT32_MIN: the sweeps
    set it for empty reads, which the upload refuses by read, and for fit; the device-side fold of the smallest such pair is
    checked on the kernels directly, below.)"""
    reads = _reads1()
    blob, off, lens = _flat(reads)
    total = len(reads) * (len(reads) - 1) // 2
    for m, u, o, e in ((37000, -37000, -37000, -37000), (38000, -2, -5, -1), (1, -38000, -5, -1), (1, -2, -70000, -1)):
        al = A.Aligner()
        al.set_scoring(m, u, o, e)
        dense_err = None
        try:
            d = _dense_on(al, mode, reads)
        except A.AlignToolsError as ex:
            dense_err = ex
        T = 0 if dense_err else int(np.median(d["score"]))
        rc, nh, out = _raw(al, mode, reads, T, total)
        if dense_err is None:
            assert rc == 0
            want = _expect(d, mode, T, len(reads))
            _same({x: out[x][:nh] for x in want}, want)
        else:
            text = al._lib.at_last_error(al._h).decode()
            assert rc == dense_err.code, (rc, text, str(dense_err))
            assert _pair_in(text) == _pair_in(str(dense_err))
        al.close()


class _PairHitsArgs(C.Structure):
    _fields_ = [("n", C.c_longlong), ("first", C.c_longlong), ("nreads", C.c_longlong),
                ("score", C.c_void_p), ("end_i", C.c_void_p), ("end_j", C.c_void_p), ("state", C.c_void_p),
                ("threshold", C.c_int), ("is_edit", C.c_int),
                ("flag", C.c_void_p), ("off", C.c_void_p), ("hits", C.c_void_p), ("cap", C.c_longlong), ("slots", C.c_void_p)]


@pytest.mark.parametrize("is_edit", (0, 1))
def test_selection_kernels_on_a_made_up_slice(is_edit):
    """at_pairhits_flag_k / at_pairhits_emit_k on dense arrays made up here: 3 001 pairs (more than one block, no multiple of the
    tile) from pair 5 000 000 011 of 200 000 reads (indices past 2^31), scores INT32_MIN at three places.  The flags, the smallest
    pair index outside the domain, the count and the records -- a / b against the closed form -- are what numpy says; a record
    buffer of 7 is never overrun."""
    import torch
    lib = A.load_library()
    rng = np.random.default_rng(5)
    n, first, nreads, T = 3001, 5_000_000_011, 200_000, 40
    score = rng.integers(0, 80, n).astype(np.int32)
    state = rng.integers(0, 4, n).astype(np.int32)
    ei = rng.integers(0, 1000, n).astype(np.int32)
    ej = rng.integers(0, 1000, n).astype(np.int32)
    bad = (2999, 1500, 777)
    for x in bad:
        score[x] = -2**31
        state[x] = 2
    keep = (state != 0) & (score != -2**31) & ((score <= T) if is_edit else (score >= T))
    assert 100 < keep.sum() < n - 100
    dev = "cuda"
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(score=score, state=state, ei=ei, ej=ej).items()}
    flag = torch.full((n,), 9, dtype=torch.int32, device=dev)
    slots = torch.full((2,), -1, dtype=torch.int64, device=dev)          # (all ones: "none")
    for cap in (n, 7):
        hits = torch.full((cap + 1, 4), GUARD, dtype=torch.int64, device=dev)   # 32-byte records and one guard row
        a = _PairHitsArgs(n, first, nreads, t["score"].data_ptr(), t["ei"].data_ptr(), t["ej"].data_ptr(), t["state"].data_ptr(), T, is_edit,
                          flag.data_ptr(), 0, hits.data_ptr(), cap, slots.data_ptr())
        torch.cuda.synchronize()
        assert lib.at_pairhits_flag_launch(C.byref(a), 256, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(flag.cpu().numpy(), keep.astype(np.int32))
        assert int(slots[0].item()) == first + min(bad)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(flag.to(torch.int64), 0)
        a.off = off.data_ptr()
        torch.cuda.synchronize()
        assert lib.at_pairhits_emit_launch(C.byref(a), 256, None) == 0
        torch.cuda.synchronize()
        assert int(slots[1].item()) == int(keep.sum())
        rec = hits.cpu().numpy()
        assert np.all(rec[cap] == GUARD)
        idx = np.nonzero(keep)[0][:cap]
        got = rec[:len(idx)].copy().view(np.int32).reshape(len(idx), 8)
        pair = rec[:len(idx), 0]
        assert np.array_equal(pair, first + idx)
        # rows before row r: r (2 n - r - 1) / 2
        ra = got[:, 2].astype(object)
        rb = got[:, 3].astype(object)
        for p, x, y in zip(pair.tolist(), ra, rb):
            assert 0 <= x < y < nreads and x * (2 * nreads - x - 1) // 2 + (y - x - 1) == p
        assert np.array_equal(got[:, 4], score[idx]) and np.array_equal(got[:, 5], ei[idx])
        assert np.array_equal(got[:, 6], ej[idx]) and np.array_equal(got[:, 7], state[idx])
