"""The argument refusals and the empty-set answers of the query-vs-target entries, through the C ABI with raw pointers (the Python
wrappers refuse some of these themselves): at_search_strands, at_scan, at_scan_local, at_scan_hits and at_allpairs_hits.

Every refusal is asserted with its return code and the WHOLE text of at_last_error, each entry's own name spelled out: the entries
share their prologue, and a shared check that named the wrong entry, or ran in another order, would show here.  The
refusals that come before any array is read are driven with NULL arrays.  No refusal reaches a kernel; the accepted calls have no
queries or no targets and launch nothing."""
import ctypes as C

import numpy as np
import pytest

import aligntools.c_amd as A

ERR_ARG, ERR_DOMAIN = A.ERR_ARG, A.ERR_DOMAIN
UNIT = (1, 1, -5, -1, -10)          # u = 1 for the edit scans; m >= 1, o <= -1, e <= -1 for the local scan
QUERY, TARGET = b"ACGTTGCA", b"GATTACAGATTACAACGTTGCAGGCCTTAAGG"
K = 2
GUARD = 0x5a5a5a5a

LIST_ENTRIES = ("at_search_strands", "at_scan", "at_scan_local")
SCAN_ENTRIES = ("at_scan", "at_scan_local", "at_scan_hits")
QT_ENTRIES = LIST_ENTRIES + ("at_scan_hits",)
WHO = {"at_search_strands": "at_search", "at_scan": "at_scan", "at_scan_local": "at_scan_local", "at_scan_hits": "at_scan_hits",
       "at_allpairs_hits": "at_allpairs_hits"}

_QT = ["nq", "q_blob", "q_off", "q_len", "nt", "t_blob", "t_off", "t_len"]
_CG = ["out_stats", "out_ncigar", "out_cigar_off", "out_cigar", "cigar_cap"]
ORDER = {
    "at_search_strands": ["mode"] + _QT + ["k", "use_cutoff", "cutoff", "strands", "out_target", "out_score", "out_end_i", "out_end_j",
                                           "out_state", "out_strand", "out_nhits"],
    "at_scan": _QT + ["k", "use_cutoff", "cutoff", "strands", "tile_cols", "flags", "out_target", "out_score", "out_end_i", "out_end_j",
                      "out_state", "out_strand", "out_nhits"] + _CG,
    "at_scan_hits": _QT + ["max_dist", "min_sep", "strands", "tile_cols", "cand_cap", "flags", "hit_cap", "out_hit_off", "out_target",
                           "out_score", "out_end_j", "out_strand"] + _CG,
    "at_allpairs_hits": ["mode", "nreads", "seq_blob", "off", "len", "first_pair", "npairs", "threshold", "chunk_pairs", "flags", "hit_cap",
                         "out_nhits", "out_pair", "out_a", "out_b", "out_score", "out_end_i", "out_end_j", "out_state"] + _CG,
}
ORDER["at_scan_local"] = ORDER["at_scan"]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(n):
    return np.full(n, GUARD, dtype=np.int32)


def _i64(n):
    return np.full(n, GUARD, dtype=np.int64)


def _args(entry, cigar=False):
    """a valid call of `entry` for one query and one target: name -> plain value or numpy array (None: a NULL pointer)"""
    a = {}
    if entry == "at_allpairs_hits":
        a.update(mode=A.MODE_LOCAL, nreads=2, seq_blob=np.frombuffer(QUERY + TARGET, dtype=np.uint8).copy(),
                 off=np.array([0, len(QUERY)], dtype=np.int64), len=np.array([len(QUERY), len(TARGET)], dtype=np.int32),
                 first_pair=0, npairs=1, threshold=5, chunk_pairs=0, flags=0, hit_cap=4, out_nhits=_i64(1), out_pair=_i64(4))
        for name in ("out_a", "out_b", "out_score", "out_end_i", "out_end_j", "out_state"):
            a[name] = _i32(4)
        n = 4
    else:
        a.update(nq=1, q_blob=np.frombuffer(QUERY, dtype=np.uint8).copy(), q_off=np.zeros(1, dtype=np.int64),
                 q_len=np.array([len(QUERY)], dtype=np.int32), nt=1, t_blob=np.frombuffer(TARGET, dtype=np.uint8).copy(),
                 t_off=np.zeros(1, dtype=np.int64), t_len=np.array([len(TARGET)], dtype=np.int32), strands=A.STRAND_FWD)
        if entry == "at_scan_hits":
            a.update(max_dist=3, min_sep=0, tile_cols=0, cand_cap=0, flags=0, hit_cap=4, out_hit_off=_i64(2))
            n = 4
        else:
            a.update(k=K, use_cutoff=0, cutoff=0, out_end_i=_i32(K), out_state=_i32(K), out_nhits=_i32(1))
            if entry == "at_search_strands":
                a.update(mode=A.MODE_LOCAL)
            else:
                a.update(tile_cols=0, flags=0)
            n = K
        for name in ("out_target", "out_score", "out_end_j", "out_strand"):
            a[name] = _i32(n)
    if "out_stats" in ORDER[entry]:
        a.update(out_stats=_i32(n * 8) if cigar else None, out_ncigar=_i32(n) if cigar else None, out_cigar_off=_i64(n + 1) if cigar else None,
                 out_cigar=np.full(64, GUARD, dtype=np.uint32) if cigar else None, cigar_cap=64 if cigar else 0)
    return a


def _call(lib, entry, handle, a):
    vals = [_p(a[name]) if a[name] is None or isinstance(a[name], np.ndarray) else a[name] for name in ORDER[entry]]
    rc = getattr(lib, entry)(handle, *vals)
    return rc, lib.at_last_error(handle).decode()


def _refused(al, entry, code, text, cigar=False, **over):
    a = _args(entry, cigar)
    a.update(over)
    got = _call(al._lib, entry, al._h, a)
    assert got == (code, text), (entry, over.keys(), got)


def _null_arrays(entry):
    """every pointer of a query-vs-target call NULL: for the refusals that read no array"""
    return {name: None for name in ORDER[entry] if name.startswith(("q_", "t_", "out_"))}


@pytest.fixture(scope="module")
def al():
    a = A.Aligner(0)
    a.set_scoring(*UNIT)
    yield a
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", QT_ENTRIES + ("at_allpairs_hits",))
def test_null_handle(al, entry):
    a = _args(entry)
    rc, text = _call(al._lib, entry, None, a)
    assert (rc, text) == (ERR_ARG, {"at_search_strands": "at_search: NULL handle", "at_scan": "at_scan: NULL handle",
                                    "at_scan_local": "at_scan_local: NULL handle", "at_scan_hits": "at_scan_hits: NULL handle",
                                    "at_allpairs_hits": "at_allpairs_hits: NULL handle"}[entry])


@pytest.mark.gpu
def test_sizes_k_strands(al):
    _refused(al, "at_search_strands", ERR_ARG, "unknown mode 9", mode=9)
    _refused(al, "at_search_strands", ERR_ARG, "at_search: negative size", nq=-1)
    _refused(al, "at_search_strands", ERR_ARG, "at_search: negative size", nt=-1)
    _refused(al, "at_scan", ERR_ARG, "at_scan: negative size", nq=-1)
    _refused(al, "at_scan", ERR_ARG, "at_scan: negative size", nt=-1)
    _refused(al, "at_scan", ERR_ARG, "at_scan: negative size", cigar_cap=-1)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: negative size", nq=-1)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: negative size", nt=-1)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: negative size", cigar_cap=-1)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: negative size", nq=-1)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: negative size", nt=-1)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: negative size", cigar_cap=-1)
    _refused(al, "at_search_strands", ERR_ARG, "at_search: k = 0 outside 1..64", k=0)
    _refused(al, "at_search_strands", ERR_ARG, "at_search: k = 65 outside 1..64", k=65)
    _refused(al, "at_scan", ERR_ARG, "at_scan: k = 0 outside 1..64", k=0)
    _refused(al, "at_scan", ERR_ARG, "at_scan: k = 65 outside 1..64", k=65)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: k = 0 outside 1..64", k=0)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: k = 65 outside 1..64", k=65)
    _refused(al, "at_search_strands", ERR_ARG, "at_search: strands = 0 outside 1..3", strands=0)
    _refused(al, "at_search_strands", ERR_ARG, "at_search: strands = 4 outside 1..3", strands=4)
    _refused(al, "at_scan", ERR_ARG, "at_scan: strands = 0 outside 1..3", strands=0)
    _refused(al, "at_scan", ERR_ARG, "at_scan: strands = 4 outside 1..3", strands=4)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: strands = 0 outside 1..3", strands=0)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: strands = 4 outside 1..3", strands=4)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: strands = 0 outside 1..3", strands=0)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: strands = 4 outside 1..3", strands=4)
    # the first failing check decides the text: the sizes before k, k before the strands, the strands before the width
    _refused(al, "at_search_strands", ERR_ARG, "at_search: negative size", nq=-1, k=0, strands=0)
    _refused(al, "at_scan", ERR_ARG, "at_scan: k = 0 outside 1..64", k=0, strands=0, tile_cols=24)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: strands = 0 outside 1..3", strands=0, tile_cols=24, flags=2)


@pytest.mark.gpu
def test_tile_cols_and_flags(al):
    _refused(al, "at_scan", ERR_ARG, "at_scan: tile_cols = 24 is not a positive multiple of 16 (or 0 for the default, 2048)", tile_cols=24)
    _refused(al, "at_scan", ERR_ARG, "at_scan: tile_cols = -16 is not a positive multiple of 16 (or 0 for the default, 2048)", tile_cols=-16)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: tile_cols = 24 is not a positive multiple of 16 (or 0 for the default, 1024)",
             tile_cols=24)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: tile_cols = -16 is not a positive multiple of 16 (or 0 for the default, 1024)",
             tile_cols=-16)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: tile_cols = 24 is not a positive multiple of 16 (or 0 for the default, 2048)",
             tile_cols=24)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: tile_cols = -16 is not a positive multiple of 16 (or 0 for the default, 2048)",
             tile_cols=-16)
    _refused(al, "at_scan", ERR_ARG, "at_scan: flags = 2 (AT_CIGAR_M or 0)", flags=2)
    _refused(al, "at_scan_local", ERR_ARG, "at_scan_local: flags = 3 (AT_CIGAR_M or 0)", flags=3)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: flags = 2 (AT_CIGAR_M or 0)", flags=2)
    _refused(al, "at_allpairs_hits", ERR_ARG, "at_allpairs_hits: flags = 2 (AT_CIGAR_M or 0)", flags=2)
    # at_scan_hits: its own checks stand between the sizes and the strands
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: max_dist = -1 is negative", max_dist=-1, strands=0)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: min_sep = -2 (a distance in columns, 0, or AT_SCAN_SEP_READ)", min_sep=-2, strands=0)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: negative capacity", cand_cap=-1, strands=0)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: negative capacity", hit_cap=-1, strands=0)
    _refused(al, "at_allpairs_hits", ERR_ARG, "at_allpairs_hits: negative capacity", hit_cap=-1, flags=2)
    _refused(al, "at_allpairs_hits", ERR_ARG, "at_allpairs_hits: negative capacity", cigar_cap=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", SCAN_ENTRIES + ("at_allpairs_hits",))
def test_cigar_outputs_all_or_none(al, entry):
    text = WHO[entry] + ": the CIGAR outputs are either all NULL or all given"
    for missing in ("out_stats", "out_ncigar", "out_cigar_off", "out_cigar"):
        _refused(al, entry, ERR_ARG, text, cigar=True, **{missing: None})
    # no words wanted: out_cigar may be NULL; the call is accepted up to the next check
    a = _args(entry, cigar=True)
    a.update(out_cigar=None, cigar_cap=0, flags=0)
    a.update({"at_allpairs_hits": dict(out_nhits=None)}.get(entry, dict(q_blob=None)))
    assert _call(al._lib, entry, al._h, a) == (ERR_ARG, WHO[entry] + ": NULL argument")


@pytest.mark.gpu
@pytest.mark.parametrize("entry", QT_ENTRIES)
def test_read_count_limits_read_no_array(al, entry):
    who = WHO[entry]
    nul = _null_arrays(entry)
    assert all(nul[name] is None for name in ("q_blob", "q_off", "q_len", "t_blob", "t_off", "t_len", "out_target", "out_score"))
    _refused(al, entry, ERR_ARG, who + ": 2147483647 queries + 1 targets: at most 2^31 - 1 reads", nq=2**31 - 1, nt=1, **nul)
    _refused(al, entry, ERR_ARG, who + ": 0 queries + 2147483648 targets: at most 2^31 - 1 reads", nq=0, nt=2**31, **nul)
    for strands in (A.STRAND_REV, A.STRAND_BOTH):
        _refused(al, entry, ERR_ARG, who + ": 0 queries, 1073741824 targets: a reverse strand needs nt < 2^30 and 2 nq + nt < 2^31",
                 nq=0, nt=2**30, strands=strands, **nul)
        _refused(al, entry, ERR_ARG, who + ": 1073741824 queries, 0 targets: a reverse strand needs nt < 2^30 and 2 nq + nt < 2^31",
                 nq=2**30, nt=0, strands=strands, **nul)
    # the forward strand alone may have 2^30 targets: the call goes on to the next check, which still reads no array
    if entry == "at_scan_hits":
        _refused(al, entry, ERR_ARG, who + ": NULL argument", nq=0, nt=2**30, **nul)
    else:
        a = _args(entry)
        a.update(nul, nq=0, nt=2**30)
        assert _call(al._lib, entry, al._h, a)[0] == 0


@pytest.mark.gpu
def test_multi_process_handle(tmp_path):
    """a handle that has joined a multi-process job (a world of one needs no collective library): the scans and at_allpairs_hits
    refuse it before they look at an array; at_search has no such check"""
    lib = A.load_library()
    other = A.Aligner(0)
    try:
        other.set_scoring(1, 2, -5, -1, -10)      # (u = 2: the scans' own check of the scoring comes behind this one)
        lib.at_comm_init.restype = C.c_int
        lib.at_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
        assert lib.at_comm_init(other._h, 0, 1, str(tmp_path).encode()) == 0, lib.at_last_error(other._h)
        for entry in SCAN_ENTRIES:
            _refused(other, entry, ERR_DOMAIN, WHO[entry] + ": one GPU only (this handle belongs to a multi-process job)", **_null_arrays(entry))
        nul = {name: None for name in ORDER["at_allpairs_hits"] if name.startswith("out_") or name in ("seq_blob", "off", "len")}
        _refused(other, "at_allpairs_hits", ERR_DOMAIN, "at_allpairs_hits: one GPU only (this handle belongs to a multi-process job)", **nul)
    finally:
        other.close()


@pytest.mark.gpu
def test_entry_specific_checks_keep_their_place():
    two = A.Aligner(0)
    try:
        two.set_scoring(1, 2, -5, -1, -10)
        # behind the read-count limits, in front of the NULL arguments
        _refused(two, "at_scan", ERR_DOMAIN, "at_scan needs the unit mismatch cost: u = 2, not 1", **_null_arrays("at_scan"))
        _refused(two, "at_scan_hits", ERR_DOMAIN, "at_scan_hits needs the unit mismatch cost: u = 2, not 1", **_null_arrays("at_scan_hits"))
        _refused(two, "at_scan", ERR_ARG, "at_scan: 2147483647 queries + 1 targets: at most 2^31 - 1 reads", nq=2**31 - 1, **_null_arrays("at_scan"))
        two.set_scoring(0, -2, -5, -1, -10)
        _refused(two, "at_scan_local", ERR_DOMAIN, "at_scan_local needs m >= 1, o <= -1 and e <= -1: m = 0, o = -5, e = -1",
                 **_null_arrays("at_scan_local"))
    finally:
        two.close()


@pytest.mark.gpu
def test_null_arguments(al):
    for entry in QT_ENTRIES:
        text = WHO[entry] + ": NULL argument"
        for name in ("q_blob", "q_off", "q_len", "t_blob", "t_off", "t_len", "out_target", "out_score"):
            _refused(al, entry, ERR_ARG, text, **{name: None})
        _refused(al, entry, ERR_ARG, text, strands=A.STRAND_REV, out_strand=None)
        _refused(al, entry, ERR_ARG, text, strands=A.STRAND_BOTH, out_strand=None)
    for entry in LIST_ENTRIES:
        for name in ("out_end_i", "out_end_j", "out_state", "out_nhits"):
            _refused(al, entry, ERR_ARG, WHO[entry] + ": NULL argument", **{name: None})
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: NULL argument", out_hit_off=None)
    _refused(al, "at_scan_hits", ERR_ARG, "at_scan_hits: NULL argument", out_end_j=None)
    for name in ("out_nhits", "seq_blob", "off", "len", "out_pair", "out_a", "out_b", "out_score", "out_end_i", "out_end_j", "out_state"):
        _refused(al, "at_allpairs_hits", ERR_ARG, "at_allpairs_hits: NULL argument", **{name: None})
    _refused(al, "at_allpairs_hits", ERR_ARG,
             "at_allpairs_hits: edit has no CIGAR here (alignments of edit distances: at_align_batch_cigar)", cigar=True, mode=A.MODE_EDIT)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", QT_ENTRIES)
def test_read_lengths_and_offsets(al, entry):
    neg32, neg64 = np.array([-1], dtype=np.int32), np.array([-1], dtype=np.int64)
    _refused(al, entry, ERR_ARG, "query 0: negative length or offset", q_len=neg32)
    _refused(al, entry, ERR_ARG, "query 0: negative length or offset", q_off=neg64)
    _refused(al, entry, ERR_ARG, "target 0: negative length or offset", t_len=neg32)
    _refused(al, entry, ERR_ARG, "target 0: negative length or offset", t_off=neg64)
    _refused(al, entry, ERR_ARG, "query 0: negative length or offset", q_len=neg32, t_len=neg32)
    zero = np.zeros(1, dtype=np.int32)
    long_q = np.array([1025], dtype=np.int32)
    if entry == "at_search_strands":
        _refused(al, entry, ERR_DOMAIN, "query 0: empty", q_len=zero)
        _refused(al, entry, ERR_DOMAIN, "target 0: empty", t_len=zero)
    elif entry == "at_scan_local":
        _refused(al, entry, ERR_DOMAIN, "query 0: empty", q_len=zero)
        _refused(al, entry, ERR_DOMAIN, "target 0: empty", t_len=zero)
        _refused(al, entry, ERR_DOMAIN, "at_scan_local: query 0 has 1025 bases: at most 1024, and max(m, u) * length < 2^20", q_len=long_q)
    else:
        _refused(al, entry, ERR_DOMAIN, WHO[entry] + ": query 0 has 1025 bases, more than 1024", q_len=long_q, t_len=neg32)


# ---------------------------------------------------------------- the accepted calls without queries or without targets

def _untouched(a, names):
    return all((a[name] == GUARD).all() for name in names if a.get(name) is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", LIST_ENTRIES)
def test_no_queries_or_no_targets_lists(al, entry):
    cigar = entry != "at_search_strands"
    outs = [name for name in ORDER[entry] if name.startswith("out_")]
    # no queries: AT_OK at once; nothing is written, no array is looked at and the configuration text stays
    before = al.last_config
    a = _args(entry, cigar)
    a.update(nq=0, q_blob=None, q_off=None, q_len=None, t_blob=None, t_off=None, t_len=None, strands=A.STRAND_BOTH)
    assert _call(al._lib, entry, al._h, a)[0] == 0
    assert _untouched(a, outs) and al.last_config == before
    # no targets: every list is empty
    for strands, text, stext in ((A.STRAND_FWD, "fwd", ""), (A.STRAND_REV, "rev", ", strands=rev"), (A.STRAND_BOTH, "both", ", strands=both")):
        a = _args(entry, cigar)
        a.update(nt=0, t_blob=None, t_off=None, t_len=None, strands=strands)
        assert _call(al._lib, entry, al._h, a)[0] == 0
        assert (a["out_target"] == -1).all() and (a["out_strand"] == -1).all() and (a["out_nhits"] == 0).all()
        assert all((a[name] == 0).all() for name in ("out_score", "out_end_i", "out_end_j", "out_state"))
        if cigar:
            assert (a["out_ncigar"] == 0).all() and (a["out_stats"] == -1).all() and (a["out_cigar_off"] == 0).all()
            assert _untouched(a, ["out_cigar"])
        assert al.last_config == {
            "at_search_strands": "search: 0 blocks, 0 slices, k=2%s; " % stext,
            "at_scan": "scan: tile=2048 overlap<=0 groups=0 k=2 strands=%s, 0 blocks, 0 slices; " % text,
            "at_scan_local": "local-scan: tile=1024 overlap<=0 tiles=0 k=2 strands=%s, 0 blocks, 0 slices; " % text}[entry]
    # a strand array is not needed for the forward strand, and is then not written
    a = _args(entry, cigar)
    a.update(nt=0, out_strand=None)
    if cigar:
        a.update(tile_cols=64)
    assert _call(al._lib, entry, al._h, a)[0] == 0 and (a["out_target"] == -1).all()
    if cigar:
        assert ": tile=64 overlap<=0 " in al.last_config


@pytest.mark.gpu
def test_no_queries_or_no_targets_hits(al):
    text = ("scan-hits: tile=2048 overlap<=0 groups=0 max_dist=3 min_sep=0 strands=%s, 0 blocks, 0 slices, candidates=0 kept=0 resweeps=0; "
            " sweep=0.000ms select=0.000ms")
    for cigar in (False, True):
        a = _args("at_scan_hits", cigar)
        # (the targets' lengths and offsets are looked through whatever nq is: they stay given)
        a.update(nq=0, q_blob=None, q_off=None, q_len=None, strands=A.STRAND_REV)
        assert _call(al._lib, "at_scan_hits", al._h, a)[0] == 0
        assert a["out_hit_off"][0] == 0 and a["out_hit_off"][1] == GUARD and al.last_config == text % "rev"
        assert _untouched(a, ["out_target", "out_score", "out_end_j", "out_strand", "out_stats", "out_ncigar", "out_cigar"])
        assert not cigar or (a["out_cigar_off"][0] == 0 and (a["out_cigar_off"][1:] == GUARD).all())
        a = _args("at_scan_hits", cigar)
        a.update(nt=0, t_blob=None, t_off=None, t_len=None)
        assert _call(al._lib, "at_scan_hits", al._h, a)[0] == 0
        assert (a["out_hit_off"] == 0).all() and al.last_config == text % "fwd"
        assert _untouched(a, ["out_target", "out_score", "out_end_j", "out_strand", "out_stats", "out_ncigar", "out_cigar"])
        assert not cigar or (a["out_cigar_off"][0] == 0 and (a["out_cigar_off"][1:] == GUARD).all())


@pytest.mark.gpu
def test_no_pairs(al):
    for cigar in (False, True):
        a = _args("at_allpairs_hits", cigar)
        a.update(npairs=0, seq_blob=None, off=None, len=None)
        assert _call(al._lib, "at_allpairs_hits", al._h, a)[0] == 0
        assert a["out_nhits"][0] == 0 and al.last_config == "allpairs-hits: threshold=5, 0 slices of <= 0 pairs, kept=0; none"
        assert _untouched(a, ["out_pair", "out_a", "out_b", "out_score", "out_end_i", "out_end_j", "out_state", "out_stats", "out_ncigar", "out_cigar"])
        assert not cigar or (a["out_cigar_off"][0] == 0 and (a["out_cigar_off"][1:] == GUARD).all())
