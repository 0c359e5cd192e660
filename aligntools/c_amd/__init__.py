"""aligntools.c_amd -- host-side mirror of the reference's function surface over
the gfx950 C-ABI shim (include/aligntools_hip.h, libaligntools_hip.so).

Mirrors reference src/alignment.h:
    opt_t / init_opt            :57-65, :102-114
    align_gla                   :417     align_local_affine   :805
    align_fit_affine_jump       :596     align_overlap        :926
    edit_dist                   :291
Every DP cell is computed by the HIP kernel; there is no CPU fallback.  If the
extension is not built, or no GPU is visible, the calls raise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AT_LIB_PATH") or os.path.join(HERE, "libaligntools_hip.so")   # (AT_LIB_PATH: A/B builds, tools/)

MODE_GLOBAL, MODE_LOCAL, MODE_FIT, MODE_OVERLAP, MODE_EDIT = 0, 1, 2, 3, 4
MODES = {"global": MODE_GLOBAL, "local": MODE_LOCAL, "fit": MODE_FIT, "overlap": MODE_OVERLAP, "edit": MODE_EDIT}
STRAND_FWD, STRAND_REV, STRAND_BOTH = 1, 2, 3
STRANDS = {"forward": STRAND_FWD, "reverse": STRAND_REV, "both": STRAND_BOTH}
OP_MID, OP_LOW, OP_UPP, OP_JUMP = 0, 1, 2, 3
CIGAR_M = 1                     # AT_CIGAR_M: '=' and 'X' merge into 'M'
CIGAR_LETTERS = b"MIDNSHP=X"    # a CIGAR word is (run length << 4) | index into this
ERR_ARG, ERR_DOMAIN = -1, -4
ST_LOW, ST_MID, ST_UPP = 1, 2, 3
SCAN_SEP_READ = -1              # AT_SCAN_SEP_READ: min_sep of Aligner.scan_hits = each query's own length

# every symbol include/aligntools_hip.h declares
ABI_SYMBOLS = ["at_init", "at_destroy", "at_last_error", "at_set_scoring", "at_set_min_score", "at_set_edit_traceback", "at_set_edit_infix", "at_align_batch",
               "at_align_batch_device", "at_align_allpairs_device", "at_render_batch_device", "at_compact_ops_device",
               "at_align_batch_strings", "at_align_allpairs", "at_align_allpairs_stream", "at_search",
               "at_search_strands", "at_scan", "at_scan_plan", "at_scan_local", "at_scan_local_plan", "at_scan_local_window", "at_scan_fit", "at_scan_fit_plan", "at_scan_fit_window", "at_scan_hits", "at_allpairs_hits", "at_revcomp", "at_revcomp_device",
               "at_cigar", "at_cigar_batch_device", "at_align_batch_cigar",
               "at_comm_init", "at_comm_broadcast_scoring", "at_comm_allgather", "at_comm_destroy", "at_comm_abi_checked",
               "at_pack_words", "at_pack_batch", "at_render", "at_last_config"]

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_lib = None
# at_allpairs_chunk_fn of include/aligntools_hip.h
ALLPAIRS_CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, _i32p, _i32p, _i32p, _i32p)


class AlignToolsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("aligntools error %d: %s" % (code, msg))
        self.code = code


def _one_hip_runtime():
    """One HIP runtime per process, whatever the import order.  PyTorch-ROCm bundles its own libamdhip64.so (same soname
    as the system one the shim is linked against); a process that loads the system runtime first and torch's second ends up
    with two, and torch then sees no GPU.  If torch is installed, its runtime is loaded here (by path, without importing
    torch) before the shim: the shim's DT_NEEDED entry then resolves to it, and a later `import torch` finds it already
    there.  Without torch (the C host, the CLI) the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def load_library():
    """Load the shim.  Raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("aligntools.c_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C aligntools/c_amd`; there is no CPU fallback" % LIB_PATH)
    _one_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    lib.at_init.restype = C.c_int
    lib.at_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    lib.at_destroy.restype = None
    lib.at_destroy.argtypes = [C.c_void_p]
    lib.at_last_error.restype = C.c_char_p
    lib.at_last_error.argtypes = [C.c_void_p]
    lib.at_last_config.restype = C.c_char_p
    lib.at_last_config.argtypes = [C.c_void_p]
    lib.at_set_scoring.restype = C.c_int
    lib.at_set_scoring.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_int]
    lib.at_set_min_score.restype = C.c_int
    lib.at_set_min_score.argtypes = [C.c_void_p, C.c_int, C.c_int32]
    lib.at_set_edit_traceback.restype = C.c_int
    lib.at_set_edit_traceback.argtypes = [C.c_void_p, C.c_int]
    lib.at_set_edit_infix.restype = C.c_int
    lib.at_set_edit_infix.argtypes = [C.c_void_p, C.c_int]
    lib.at_align_batch.restype = C.c_int
    lib.at_align_batch.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]
    lib.at_align_batch_device.restype = C.c_int
    lib.at_align_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    lib.at_align_allpairs_device.restype = C.c_int
    lib.at_align_allpairs_device.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.at_render_batch_device.restype = C.c_int
    lib.at_render_batch_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p]
    lib.at_compact_ops_device.restype = C.c_int
    lib.at_compact_ops_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]
    lib.at_align_batch_strings.restype = C.c_int
    lib.at_align_batch_strings.argtypes = [C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 13
    lib.at_align_allpairs.restype = C.c_int
    lib.at_align_allpairs.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.at_align_allpairs_stream.restype = C.c_int
    lib.at_align_allpairs_stream.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                             ALLPAIRS_CHUNK_FN, C.c_void_p]
    lib.at_search.restype = C.c_int
    lib.at_search.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_int, C.c_int, C.c_int32] + [C.c_void_p] * 6
    lib.at_search_strands.restype = C.c_int
    lib.at_search_strands.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int] + [C.c_void_p] * 7
    lib.at_scan.restype = C.c_int
    lib.at_scan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_int, C.c_int, C.c_int32, C.c_int, C.c_int32, C.c_int] + [C.c_void_p] * 11 + [C.c_int64]
    lib.at_scan_local.restype = C.c_int
    lib.at_scan_local.argtypes = lib.at_scan.argtypes
    lib.at_scan_local_plan.restype = C.c_int
    lib.at_scan_local_plan.argtypes = [C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i64p, _i64p]
    lib.at_scan_local_window.restype = C.c_int64
    lib.at_scan_local_window.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.at_scan_fit.restype = C.c_int
    lib.at_scan_fit.argtypes = lib.at_scan.argtypes
    lib.at_scan_fit_plan.restype = C.c_int
    lib.at_scan_fit_plan.argtypes = lib.at_scan_local_plan.argtypes
    lib.at_scan_fit_window.restype = C.c_int
    lib.at_scan_fit_window.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, _i64p, _i64p]
    lib.at_scan_hits.restype = C.c_int
    lib.at_scan_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_int64, C.c_int, C.c_int64] + [C.c_void_p] * 9 + [C.c_int64]
    lib.at_allpairs_hits.restype = C.c_int
    lib.at_allpairs_hits.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64,
                                     C.c_int, C.c_int64] + [C.c_void_p] * 12 + [C.c_int64]
    lib.at_scan_plan.restype = C.c_int
    lib.at_scan_plan.argtypes = [C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_int32, _i32p, _i32p, _i64p]
    lib.at_revcomp.restype = C.c_int
    lib.at_revcomp.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.at_revcomp_device.restype = C.c_int
    lib.at_revcomp_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.at_comm_abi_checked.restype = C.c_int
    lib.at_comm_abi_checked.argtypes = []
    lib.at_pack_words.restype = C.c_int64
    lib.at_pack_words.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    lib.at_pack_batch.restype = C.c_int
    lib.at_pack_batch.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.at_render.restype = C.c_int
    lib.at_render.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.at_cigar.restype = C.c_int
    lib.at_cigar.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.at_cigar_batch_device.restype = C.c_int
    lib.at_cigar_batch_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 4 + [
        C.c_int64, C.c_void_p]
    lib.at_align_batch_cigar.restype = C.c_int
    lib.at_align_batch_cigar.argtypes = [C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 8 + [C.c_int64]
    _lib = lib
    return lib


def kernel_source_sha16():
    """Fingerprint of the SWEEP kernels' sources -- at_sweep.hip.h, at_sweep16.hip.h, at_walk16.hip.h, at_myers.hip.h, at_launch.h and the instantiation
    units at_k*.hip / at_myers.hip; not the packing / rendering kernels nor the host-side plumbing (at_hip.hip, at_comm.hip), whose
    choices show in the kernel configuration string: the committed PMC counters under profiles/ belong to one state of those
    kernels, and bench.py prices its roofline with them only while this fingerprint still matches."""
    import hashlib
    d = os.path.join(HERE, "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name in ("at_sweep.hip.h", "at_sweep16.hip.h", "at_walk16.hip.h", "at_myers.hip.h", "at_launch.h", "at_myers.hip") or (name.startswith("at_k") and name.endswith(".hip")):
            h.update(name.encode() + b"\0")
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


class opt_t:
    """The reference's scoring block with its defaults (init_opt, alignment.h:102-114)."""

    def __init__(self, m=1, u=-2, o=-5, e=-1, j=-10, s=False, sites=None):
        self.m, self.u, self.o, self.e, self.j, self.s = m, u, o, e, j, bool(s)
        self.sites = list(sites or [])


def init_opt():
    return opt_t()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pack_pairs(pairs, bits=0):
    """Host helper: list of (s1, s2) bytes -> (words, woff1, woff2, len1, len2, bits)."""
    lib = load_library()
    blob, off1, len1, off2, len2 = _flatten(pairs)
    n = len(pairs)
    b = C.c_int(0)
    rc = lib.at_pack_batch(n, _ptr(blob), _ptr(off1), _ptr(len1), _ptr(off2), _ptr(len2), bits, C.byref(b), None,
                           _ptr(off1), _ptr(off2))
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    nw = lib.at_pack_words(n, _ptr(len1), _ptr(len2), b.value)
    words = np.zeros(nw, dtype=np.uint32)
    woff1 = np.zeros(n, dtype=np.int64)
    woff2 = np.zeros(n, dtype=np.int64)
    rc = lib.at_pack_batch(n, _ptr(blob), _ptr(off1), _ptr(len1), _ptr(off2), _ptr(len2), b.value, None,
                           _ptr(words), _ptr(woff1), _ptr(woff2))
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    return words, woff1, woff2, len1, len2, b.value


def revcomp(s):
    """Host helper: the reverse complement of a str / bytes as bytes (at_revcomp: IUPAC codes in both letter cases, every
    other byte unchanged)."""
    lib = load_library()
    s = _b(s)
    out = C.create_string_buffer(len(s) + 1)
    rc = lib.at_revcomp(s, len(s), out)
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    return out.raw[:len(s)]


def scan_plan(len1, len2, cutoff=None, tile_cols=0):
    """Host helper (at_scan_plan): how Aligner.scan cuts a pair of len1 x len2 -- (tile, overlap, ngroups): the columns a lane owns,
    the warm-up columns in front of a tile and the groups of 64 tiles."""
    lib = load_library()
    tile, ov, ng = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    rc = lib.at_scan_plan(int(len1), int(len2), 0 if cutoff is None else 1, 0 if cutoff is None else int(cutoff), int(tile_cols),
                          C.byref(tile), C.byref(ov), C.byref(ng))
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    return tile.value, ov.value, ng.value


def scan_local_plan(len1, len2, m, u, o, e, min_score=None, tile_cols=0):
    """Host helper (at_scan_local_plan): how Aligner.scan_local cuts a pair of len1 x len2 under the scoring m / u / o / e --
    (tile, overlap, ntiles, nfull): the columns a tile owns, the columns in front of them, the tiles of the target and how many of
    them (the leading ones) have the full shape len1 x (tile + overlap).  Tile n sweeps the target columns
    (max(0, n * tile - overlap), min(len2, that + tile + overlap)]."""
    lib = load_library()
    tile, ov, nt, nf = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rc = lib.at_scan_local_plan(int(len1), int(len2), 0 if min_score is None else 1, 0 if min_score is None else int(min_score),
                                int(tile_cols), int(m), int(u), int(o), int(e), C.byref(tile), C.byref(ov), C.byref(nt), C.byref(nf))
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    return tile.value, ov.value, nt.value, nf.value


def scan_local_window(end_i, end_j, score, m, u, o, e):
    """Host helper (at_scan_local_window): ws of a hit of Aligner.scan_local -- its alignment lies in the target columns (ws, end_j]."""
    return int(load_library().at_scan_local_window(int(end_i), int(end_j), int(score), int(m), int(u), int(o), int(e)))


def scan_fit_plan(len1, len2, m, u, o, e, min_score=None, tile_cols=0):
    """Host helper (at_scan_fit_plan): how Aligner.scan_fit cuts a pair of len1 x len2 under the scoring m / u / o / e --
    (tile, overlap, ntiles, nfull): the end columns a tile owns (tile n: n * tile <= j < (n + 1) * tile), the columns in front of
    them, the tiles of the target (0 for len2 < len1) and how many of them (the leading ones) have the full shape
    len1 x (tile + overlap).  Tile n sweeps the target columns (max(0, n * tile - overlap), min(len2, that + tile + overlap)]; the
    tiles 1 .. min(ntiles - 1, overlap // tile) would repeat tile 0's sweep and are not swept."""
    lib = load_library()
    tile, ov, nt, nf = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rc = lib.at_scan_fit_plan(int(len1), int(len2), 0 if min_score is None else 1, 0 if min_score is None else int(min_score),
                              int(tile_cols), int(m), int(u), int(o), int(e), C.byref(tile), C.byref(ov), C.byref(nt), C.byref(nf))
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    return tile.value, ov.value, nt.value, nf.value


def scan_fit_window(end_j, score, len1, len2, m, u, o, e):
    """Host helper (at_scan_fit_window): (ws, we) of a hit of Aligner.scan_fit -- the fit pair (query, target columns (ws, we]) has
    the hit's score and state, the end column end_j - ws and its ops."""
    lib = load_library()
    ws, we = C.c_int64(0), C.c_int64(0)
    rc = lib.at_scan_fit_window(int(end_j), int(score), int(len1), int(len2), int(m), int(u), int(o), int(e), C.byref(ws), C.byref(we))
    if rc:
        raise AlignToolsError(rc, lib.at_last_error(None).decode())
    return ws.value, we.value


def cigar(ops, s1, end_i, s2, end_j, extended=True):
    """Host helper (at_cigar): ops (END -> START) + end cell -> (words, stats): the run-length CIGAR as a numpy uint32 array of
    (run length << 4) | BAM op code, in reading order, and the eight statistics (start_i, start_j, equal, unequal, I bases, D bases,
    N bases, I runs + D runs) as a numpy int32 array.  extended: '=' / 'X'; else both are 'M'."""
    lib = load_library()
    ops, s1, s2 = bytes(ops), _b(s1), _b(s2)
    words = np.zeros(max(1, len(ops)), dtype=np.uint32)
    stats = np.zeros(8, dtype=np.int32)
    nc = C.c_int32(0)
    rc = lib.at_cigar(ops, len(ops), s1, int(end_i), s2, int(end_j), 0 if extended else CIGAR_M, _ptr(words), C.byref(nc), _ptr(stats))
    if rc:
        raise AlignToolsError(rc, "at_cigar: " + ("ops inconsistent with the sequences" if rc == ERR_DOMAIN else "bad argument"))
    return words[:nc.value].copy(), stats


def cigar_string(words):
    """CIGAR words -> text, for example b"12=1X3I40="."""
    return b"".join(b"%d%c" % (int(w) >> 4, CIGAR_LETTERS[int(w) & 15]) for w in words)


def _flatten(pairs):
    n = len(pairs)
    len1 = np.fromiter((len(p[0]) for p in pairs), dtype=np.int32, count=n)
    len2 = np.fromiter((len(p[1]) for p in pairs), dtype=np.int32, count=n)
    tot = len1.astype(np.int64) + len2
    starts = np.zeros(n, dtype=np.int64)
    if n > 1:
        np.cumsum(tot[:-1], out=starts[1:])
    off1 = starts
    off2 = starts + len1
    blob = np.frombuffer(b"".join(p[0] + p[1] for p in pairs) + b"\0", dtype=np.uint8).copy()
    return blob, off1, len1, off2, len2


def _b(s):
    return s.encode("latin1") if isinstance(s, str) else bytes(s)


class Aligner:
    """One handle = one GPU (one process per GPU)."""

    def __init__(self, device=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        self._edit_tb = False
        ids = None if device is None else (C.c_int * 1)(int(device))
        rc = self._lib.at_init(ids, 1 if device is not None else 0, C.byref(self._h))
        if rc:
            raise AlignToolsError(rc, self._lib.at_last_error(None).decode())

    def close(self):
        if self._h:
            self._lib.at_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise AlignToolsError(rc, self._lib.at_last_error(self._h).decode())

    @property
    def last_config(self):
        return self._lib.at_last_config(self._h).decode()

    def set_scoring(self, m=1, u=-2, o=-5, e=-1, j=-10, use_jump=False, sites=None):
        sites = list(sites or [])
        arr = (C.c_int * max(1, len(sites)))(*sites)
        self._check(self._lib.at_set_scoring(self._h, m, u, o, e, j, 1 if use_jump else 0, arr, len(sites)))

    def set_opt(self, opt):
        self.set_scoring(opt.m, opt.u, opt.o, opt.e, opt.j, opt.s, opt.sites)

    def set_min_score(self, min_score=None):
        """All-vs-all overlap scores: pairs proven to score below `min_score` are not swept (state 0, score = an upper bound);
        None switches the threshold off (at_set_min_score)."""
        self._check(self._lib.at_set_min_score(self._h, 0 if min_score is None else 1, 0 if min_score is None else int(min_score)))

    def set_edit_traceback(self, on=True):
        """Edit alignments (at_set_edit_traceback): with it on, align_batch("edit", ...) returns `ops` (and r1 / r2 with render),
        and align_batch_strings / align_batch_cigar accept "edit".  Needs u == 1, pure ACGT, first sequences of up to 1 024 and
        second ones of up to 3 792 bases; outside that domain the calls raise.  Off (the default): edit returns the number only."""
        self._check(self._lib.at_set_edit_traceback(self._h, 1 if on else 0))
        self._edit_tb = bool(on)

    def set_edit_infix(self, on=True):
        """Edit infix mode (at_set_edit_infix): with it on, "edit" is the distance of the best match of s1 INSIDE s2 -- D(0,j) = 0,
        score = min over j of D(l1,j), end cell (l1, j*) with the smallest such j -- in align_batch, align_batch_strings,
        align_batch_cigar, cigar and search(..., strands=...); ops (with set_edit_traceback) run from (l1, j*) to (0, j0).  The
        domain is that of the edit alignments; outside it, and in align_allpairs, the calls raise (never the global number).
        Off (the default): edit is the global distance."""
        self._check(self._lib.at_set_edit_infix(self._h, 1 if on else 0))

    def align_batch_strings(self, mode, pairs):
        """pairs: list of (s1, s2) bytes/str.  The two gapped strings of every pair, rendered on the GPU
        (at_align_batch_strings).  Returns a dict: score, end_i, end_j, state, nops (numpy) and r1, r2 (lists of str)."""
        if isinstance(mode, str):
            mode = MODES[mode]
        pairs = [(_b(a), _b(b)) for a, b in pairs]
        n = len(pairs)
        blob, off1, len1, off2, len2 = _flatten(pairs)
        score, end_i, end_j, state, nops = (np.zeros(n, dtype=np.int32) for _ in range(5))
        str_off = off1 + np.arange(n, dtype=np.int64)          # slots of l1+l2+1 bytes
        total = int(len(blob) + n + 64)
        r1 = np.zeros(total, dtype=np.uint8)
        r2 = np.zeros(total, dtype=np.uint8)
        self._check(self._lib.at_align_batch_strings(self._h, mode, n, _ptr(blob), _ptr(off1), _ptr(len1), _ptr(off2),
                                                     _ptr(len2), _ptr(score), _ptr(end_i), _ptr(end_j), _ptr(state),
                                                     _ptr(r1), _ptr(r2), _ptr(str_off), _ptr(nops)))
        b1, b2 = r1.tobytes(), r2.tobytes()
        out = dict(score=score, end_i=end_i, end_j=end_j, state=state, nops=nops)
        out["r1"] = [b1[str_off[k]:str_off[k] + nops[k]].decode("latin1") for k in range(n)]
        out["r2"] = [b2[str_off[k]:str_off[k] + nops[k]].decode("latin1") for k in range(n)]
        return out

    def render_batch_device(self, npairs, d_seq, bits, d_woff1, d_woff2, d_end_i, d_end_j, d_ops, d_ops_off, d_nops,
                            d_r1, d_r2, d_str_off=None, nul_terminate=False, stream=0):
        """Raw device-pointer entry of the rendering kernel (at_render_batch_device)."""
        self._check(self._lib.at_render_batch_device(self._h, npairs, d_seq, bits, d_woff1, d_woff2, d_end_i, d_end_j,
                                                     d_ops, d_ops_off, d_nops, d_r1, d_r2, d_str_off,
                                                     1 if nul_terminate else 0, stream))

    def compact_ops_device(self, npairs, d_ops, d_ops_off, d_nops, d_packed, packed_cap, d_packed_off, stream=0):
        """Slots of ops -> one contiguous payload + exclusive offsets (at_compact_ops_device)."""
        self._check(self._lib.at_compact_ops_device(self._h, npairs, d_ops, d_ops_off, d_nops, d_packed, packed_cap,
                                                    d_packed_off, stream))

    def cigar_batch_device(self, npairs, d_seq, bits, d_woff1, d_woff2, d_end_i, d_end_j, d_ops, d_ops_off, d_nops,
                           d_ncigar, d_stats, d_cigar_off, d_cigar, cigar_cap, extended=True, stream=0):
        """Raw device-pointer entry of the CIGAR kernel (at_cigar_batch_device)."""
        self._check(self._lib.at_cigar_batch_device(self._h, npairs, d_seq, bits, d_woff1, d_woff2, d_end_i, d_end_j,
                                                    d_ops, d_ops_off, d_nops, 0 if extended else CIGAR_M, d_ncigar, d_stats,
                                                    d_cigar_off, d_cigar, cigar_cap, stream))

    def align_batch_cigar(self, mode, pairs, extended=True):
        """pairs: list of (s1, s2) bytes/str.  CIGARs and statistics made on the GPU (at_align_batch_cigar).  Returns a dict: score,
        end_i, end_j, state, ncigar (numpy), stats (numpy int32 [n, 8]), cigar_off (numpy int64 [n + 1]) and cigar, a list of
        numpy uint32 arrays of (run length << 4) | BAM op code in reading order."""
        if isinstance(mode, str):
            mode = MODES[mode]
        pairs = [(_b(a), _b(b)) for a, b in pairs]
        n = len(pairs)
        blob, off1, len1, off2, len2 = _flatten(pairs)
        score, end_i, end_j, state, ncigar = (np.zeros(n, dtype=np.int32) for _ in range(5))
        stats = np.zeros((n, 8), dtype=np.int32)
        cigar_off = np.zeros(n + 1, dtype=np.int64)
        cap = 16 * n + 64                                      # a second call if the batch has more runs than that
        for _ in range(2):
            words = np.zeros(cap, dtype=np.uint32)
            self._check(self._lib.at_align_batch_cigar(self._h, mode, n, _ptr(blob), _ptr(off1), _ptr(len1), _ptr(off2), _ptr(len2),
                                                       0 if extended else CIGAR_M, _ptr(score), _ptr(end_i), _ptr(end_j),
                                                       _ptr(state), _ptr(stats), _ptr(ncigar), _ptr(cigar_off), _ptr(words), cap))
            if cigar_off[n] <= cap:
                break
            cap = int(cigar_off[n])
        out = dict(score=score, end_i=end_i, end_j=end_j, state=state, ncigar=ncigar, stats=stats, cigar_off=cigar_off)
        out["cigar"] = [words[cigar_off[k]:cigar_off[k] + ncigar[k]].copy() for k in range(n)]
        return out

    def align_batch(self, mode, pairs, traceback=True, render=True):
        """pairs: list of (s1, s2) bytes/str.  Returns a dict of numpy arrays
        (score, end_i, end_j, state, nops), `ops` (list of bytes, END->START) and,
        with render, `r1`/`r2` (the reference's two gapped strings, rendered on the host by at_render;
        align_batch_strings renders them on the GPU)."""
        if isinstance(mode, str):
            mode = MODES[mode]
        pairs = [(_b(a), _b(b)) for a, b in pairs]
        n = len(pairs)
        blob, off1, len1, off2, len2 = _flatten(pairs)
        tb = bool(traceback) and (mode != MODE_EDIT or getattr(self, "_edit_tb", False))
        score = np.zeros(n, dtype=np.int32)
        end_i = np.zeros(n, dtype=np.int32)
        end_j = np.zeros(n, dtype=np.int32)
        state = np.zeros(n, dtype=np.int32)
        nops = np.zeros(n, dtype=np.int32)
        ops_off = off1.copy()          # l1+l2 bytes per pair, same offsets as the blob
        ops = np.zeros(len(blob) + 64, dtype=np.uint8) if tb else None
        self._check(self._lib.at_align_batch(self._h, mode, n, _ptr(blob), _ptr(off1), _ptr(len1), _ptr(off2), _ptr(len2),
                                             1 if tb else 0, _ptr(score), _ptr(end_i), _ptr(end_j), _ptr(state),
                                             _ptr(ops), _ptr(ops_off) if tb else None, _ptr(nops) if tb else None))
        out = dict(score=score, end_i=end_i, end_j=end_j, state=state, nops=nops)
        if tb:
            out["ops"] = [bytes(ops[ops_off[k]:ops_off[k] + nops[k]]) for k in range(n)]
            if render:
                r1s, r2s = [], []
                for k in range(n):
                    a, b = self.render(out["ops"][k], pairs[k][0], int(end_i[k]), pairs[k][1], int(end_j[k]))
                    r1s.append(a)
                    r2s.append(b)
                out["r1"], out["r2"] = r1s, r2s
        return out

    def render(self, ops, s1, end_i, s2, end_j):
        n = len(ops)
        r1 = C.create_string_buffer(n + 1)
        r2 = C.create_string_buffer(n + 1)
        rc = self._lib.at_render(ops, n, s1, end_i, s2, end_j, r1, r2)
        if rc:
            raise AlignToolsError(rc, "at_render: ops inconsistent with the sequences")
        return r1.raw[:n].decode("latin1"), r2.raw[:n].decode("latin1")

    # raw device-pointer entry (bench.py): all arguments are integer device addresses
    def align_batch_device(self, mode, npairs, d_seq, bits, d_woff1, d_len1, d_woff2, d_len2, max_len1, max_len2,
                           uniform_shape, want_traceback, d_score, d_end_i, d_end_j, d_state, d_ops, d_ops_off, d_nops, stream=0):
        self._check(self._lib.at_align_batch_device(self._h, mode, npairs, d_seq, bits, d_woff1, d_len1, d_woff2, d_len2,
                                                    max_len1, max_len2, 1 if uniform_shape else 0,
                                                    1 if want_traceback else 0, d_score, d_end_i,
                                                    d_end_j, d_state, d_ops, d_ops_off, d_nops, stream))


    def align_allpairs_stream(self, mode, reads_blob, off, lens, first_pair, npairs, chunk_pairs, on_slice):
        """All-vs-all scores in slices with bounded memory (at_align_allpairs_stream): reads_blob uint8, off int64, lens int32
        (numpy); on_slice(first, score, end_i, end_j, state) gets numpy views that are valid during the call only."""
        if isinstance(mode, str):
            mode = MODES[mode]
        err = []

        def cb(_user, first, n, sc, ei, ej, st):
            try:
                on_slice(int(first), *(np.ctypeslib.as_array(x, shape=(int(n),)) for x in (sc, ei, ej, st)))
                return 0
            except BaseException as ex:   # (an exception must not unwind through the C frames)
                err.append(ex)
                return 1
        fn = ALLPAIRS_CHUNK_FN(cb)
        rc = self._lib.at_align_allpairs_stream(self._h, mode, len(lens), _ptr(reads_blob), _ptr(off), _ptr(lens), first_pair, npairs,
                                                chunk_pairs, fn, None)
        if err:
            raise err[0]
        self._check(rc)

    def revcomp_device(self, nseq, d_seq, bits, d_woff, d_len, d_out, d_out_woff=None, stream=0):
        """Raw device-pointer entry of the reverse-complement kernel for packed reads (at_revcomp_device)."""
        self._check(self._lib.at_revcomp_device(self._h, nseq, d_seq, bits, d_woff, d_len, d_out, d_out_woff, stream))

    def search(self, mode, queries, targets, k=1, cutoff=None, strands="forward"):
        """Every query against every target, the best `k` (1..64) hits of each query (at_search).  queries / targets: lists of
        str or bytes.  Rank: higher score first (edit: smaller distance first), ties: smaller target index first; `cutoff` keeps
        only hits with score >= cutoff (edit: distance <= cutoff).  fit: targets shorter than a query are not its candidates.
        Returns a dict: target, score, end_i, end_j, state -- int32 arrays of shape (nq, k), row q = the hits of query q in rank
        order, unused entries with target -1 -- and nhits (nq,).
        strands: "forward" (the queries as given), "reverse" (their reverse complements, made on the device) or "both"
        (at_search_strands).  With "reverse" / "both" a hit is (target, strand) and the dict also holds `strand` (nq, k): 0 = the
        query as given, 1 = its reverse complement (score, end cell and state are those of align_batch on (revcomp(query),
        target)), -1 = unused; ties on score and target rank strand 0 first."""
        if isinstance(mode, str):
            mode = MODES[mode]
        if strands not in STRANDS:
            raise ValueError("strands must be one of %s" % ", ".join(sorted(STRANDS)))
        qs = [_b(x) for x in queries]
        ts = [_b(x) for x in targets]
        nq, nt = len(qs), len(ts)

        def pack(seqs):
            lens = np.fromiter((len(x) for x in seqs), dtype=np.int32, count=len(seqs))
            off = np.zeros(len(seqs), dtype=np.int64)
            if len(seqs) > 1:
                np.cumsum(lens[:-1], out=off[1:])
            return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy(), off, lens
        qb, qo, ql = pack(qs)
        tb, to, tl = pack(ts)
        out = {name: np.full((nq, int(k)), -1 if name == "target" else 0, dtype=np.int32)
               for name in ("target", "score", "end_i", "end_j", "state")}
        nhits = np.zeros(nq, dtype=np.int32)
        if strands != "forward":
            out["strand"] = np.full((nq, int(k)), -1, dtype=np.int32)
            self._check(self._lib.at_search_strands(self._h, mode, nq, _ptr(qb), _ptr(qo), _ptr(ql), nt, _ptr(tb), _ptr(to), _ptr(tl),
                                                    int(k), 0 if cutoff is None else 1, 0 if cutoff is None else int(cutoff),
                                                    STRANDS[strands], _ptr(out["target"]), _ptr(out["score"]), _ptr(out["end_i"]),
                                                    _ptr(out["end_j"]), _ptr(out["state"]), _ptr(out["strand"]), _ptr(nhits)))
            out["nhits"] = nhits
            return out
        self._check(self._lib.at_search(self._h, mode, nq, _ptr(qb), _ptr(qo), _ptr(ql), nt, _ptr(tb), _ptr(to), _ptr(tl), int(k),
                                        0 if cutoff is None else 1, 0 if cutoff is None else int(cutoff),
                                        _ptr(out["target"]), _ptr(out["score"]), _ptr(out["end_i"]), _ptr(out["end_j"]),
                                        _ptr(out["state"]), _ptr(nhits)))
        out["nhits"] = nhits
        return out

    def scan(self, queries, targets, k=1, cutoff=None, strands="forward", cigar=False, cigar_m=False, tile_cols=0):
        """Reads against long targets (at_scan): for every query the best `k` hits over the targets, a hit being the best match of
        the query inside a target under the rule of set_edit_infix -- whatever that setting says -- with no bound on the target
        length.  Queries of up to 1 024 bases, ACGT, u == 1.  Returns the dict of search("edit", ...) (end_j is the absolute
        column; `strand` with "reverse" / "both") and, with cigar=True, per hit entry stats (nq, k, 8), ncigar (nq, k) and cigar, a
        list of nq lists of k numpy uint32 arrays ('=' / 'X'; cigar_m: 'M'); an unused entry has no runs and a row of -1.
        tile_cols: the columns a lane owns (a multiple of 16; 0: the default) -- the results do not depend on it."""
        return self._scan_call("at_scan", queries, targets, k, cutoff, strands, cigar, cigar_m, tile_cols)

    def _scan_call(self, entry, queries, targets, k, cutoff, strands, cigar, cigar_m, tile_cols):
        """at_scan / at_scan_local / at_scan_fit: one argument list, one layout of the results"""
        if strands not in STRANDS:
            raise ValueError("strands must be one of %s" % ", ".join(sorted(STRANDS)))
        qs = [_b(x) for x in queries]
        ts = [_b(x) for x in targets]
        nq, nt, k = len(qs), len(ts), int(k)

        def pack(seqs):
            lens = np.fromiter((len(x) for x in seqs), dtype=np.int32, count=len(seqs))
            off = np.zeros(len(seqs), dtype=np.int64)
            if len(seqs) > 1:
                np.cumsum(lens[:-1], out=off[1:])
            return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy(), off, lens
        qb, qo, ql = pack(qs)
        tb, to, tl = pack(ts)
        kk = max(k, 0)
        out = {name: np.full((nq, kk), -1 if name == "target" else 0, dtype=np.int32)
               for name in ("target", "score", "end_i", "end_j", "state")}
        nhits = np.zeros(nq, dtype=np.int32)
        strand = np.full((nq, kk), -1, dtype=np.int32)
        n = nq * kk
        stats = np.full((nq, kk, 8), -1, dtype=np.int32) if cigar else None
        ncigar = np.zeros((nq, kk), dtype=np.int32) if cigar else None
        cigar_off = np.zeros(n + 1, dtype=np.int64) if cigar else None
        cap = 16 * n + 64                                      # a second call if the hits have more runs than that
        for _ in range(2):
            words = np.zeros(cap, dtype=np.uint32) if cigar else None
            self._check(getattr(self._lib, entry)(self._h, nq, _ptr(qb), _ptr(qo), _ptr(ql), nt, _ptr(tb), _ptr(to), _ptr(tl), k,
                                          0 if cutoff is None else 1, 0 if cutoff is None else int(cutoff), STRANDS[strands],
                                          int(tile_cols), CIGAR_M if cigar_m else 0, _ptr(out["target"]), _ptr(out["score"]),
                                          _ptr(out["end_i"]), _ptr(out["end_j"]), _ptr(out["state"]), _ptr(strand), _ptr(nhits),
                                          _ptr(stats), _ptr(ncigar), _ptr(cigar_off), _ptr(words), cap if cigar else 0))
            if not cigar or cigar_off[n] <= cap:
                break
            cap = int(cigar_off[n])
        if strands != "forward":
            out["strand"] = strand
        out["nhits"] = nhits
        if cigar:
            out["stats"], out["ncigar"], out["cigar_off"] = stats, ncigar, cigar_off
            out["cigar"] = [[words[cigar_off[q * kk + e]:cigar_off[q * kk + e] + max(int(ncigar[q, e]), 0)].copy() for e in range(kk)]
                            for q in range(nq)]
        return out

    def scan_local(self, queries, targets, k=1, min_score=None, strands="forward", cigar=False, cigar_m=False, tile_cols=0):
        """Smith-Waterman of reads against long targets (at_scan_local): for every query the best `k` hits over the targets, one per
        (query, strand, target), a hit being exactly what align_batch("local", ...) returns for (query or its reverse complement,
        target) -- score, end cell, state -- with no bound on the target length.  Scoring with m >= 1, o <= -1, e <= -1; queries of
        1 .. 1 024 bases.  min_score keeps only hits with score >= min_score.  Returns what scan() returns: the dict of
        search("local", ...) (end_j is the absolute column; `strand` with "reverse" / "both") and, with cigar=True, stats, ncigar and
        cigar as scan() lays them out.  tile_cols: the columns a tile owns (a multiple of 16; 0: the default) -- the results do not
        depend on it."""
        return self._scan_call("at_scan_local", queries, targets, k, min_score, strands, cigar, cigar_m, tile_cols)

    def scan_fit(self, queries, targets, k=1, min_score=None, strands="forward", cigar=False, cigar_m=False, tile_cols=0):
        """End-to-end affine alignment of reads against long targets (at_scan_fit): for every query the best `k` hits over the
        targets, one per (query, strand, target), a hit being exactly what align_batch("fit", ...) returns without jump sites for
        (query or its reverse complement, target) -- score, end cell (len(query), j*), state ST_MID or ST_LOW -- with no bound on
        the target length; a target shorter than the query is no candidate.  Scoring with m >= 1, o <= -1, e <= -1, no jump sites;
        queries of 1 .. 1 024 bases.  min_score keeps only hits with score >= min_score.  Returns what scan() returns: the dict of
        search("fit", ...) (end_j is the absolute column; `strand` with "reverse" / "both") and, with cigar=True, stats, ncigar and
        cigar as scan() lays them out.  tile_cols: the end columns a tile owns (a multiple of 16; 0: the default) -- the results
        do not depend on it."""
        return self._scan_call("at_scan_fit", queries, targets, k, min_score, strands, cigar, cigar_m, tile_cols)

    def scan_hits(self, queries, targets, max_dist, min_sep=SCAN_SEP_READ, strands="forward", cigar=False, cigar_m=False, tile_cols=0,
                  cand_cap=0):
        """Every occurrence of every query in every target with at most `max_dist` edits (at_scan_hits): the leftmost column of each
        strict local minimum of the last row of scan()'s table that is <= min(max_dist, len(query) - 1).  min_sep > 0 keeps an
        occurrence only if no other occurrence of the same (query, strand, target) within min_sep columns is better -- smaller
        distance, then smaller column; 0 keeps all; SCAN_SEP_READ (-1, the default) stands for each query's own length.
        Returns a dict: hit_off (nq + 1,) int64 -- the hits of query q are the entries hit_off[q] .. hit_off[q + 1] -- and target,
        score, end_j (the absolute end column), strand (0 / 1), int32 arrays over the hits, a query's hits by (distance, target,
        strand, column); with cigar=True also stats (nhits, 8), ncigar (nhits,) and cigar, a list of numpy uint32 arrays
        ('=' / 'X'; cigar_m: 'M').  tile_cols and cand_cap (the candidate records a slice may leave on the device; 0: the default)
        do not change the results."""
        if strands not in STRANDS:
            raise ValueError("strands must be one of %s" % ", ".join(sorted(STRANDS)))
        qs = [_b(x) for x in queries]
        ts = [_b(x) for x in targets]
        nq, nt = len(qs), len(ts)

        def pack(seqs):
            lens = np.fromiter((len(x) for x in seqs), dtype=np.int32, count=len(seqs))
            off = np.zeros(len(seqs), dtype=np.int64)
            if len(seqs) > 1:
                np.cumsum(lens[:-1], out=off[1:])
            return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy(), off, lens
        qb, qo, ql = pack(qs)
        tb, to, tl = pack(ts)
        hit_off = np.zeros(nq + 1, dtype=np.int64)
        hit_cap, cap = 4 * nq + 64, 0
        for _ in range(3):                                      # more hits, then more runs, than the first guess has room for
            out = {name: np.zeros(hit_cap, dtype=np.int32) for name in ("target", "score", "end_j", "strand")}
            stats = np.full((hit_cap, 8), -1, dtype=np.int32) if cigar else None
            ncigar = np.zeros(hit_cap, dtype=np.int32) if cigar else None
            cigar_off = np.zeros(hit_cap + 1, dtype=np.int64) if cigar else None
            cap = max(cap, 16 * hit_cap + 64)
            words = np.zeros(cap, dtype=np.uint32) if cigar else None
            self._check(self._lib.at_scan_hits(self._h, nq, _ptr(qb), _ptr(qo), _ptr(ql), nt, _ptr(tb), _ptr(to), _ptr(tl), int(max_dist),
                                               int(min_sep), STRANDS[strands], int(tile_cols), int(cand_cap), CIGAR_M if cigar_m else 0,
                                               hit_cap, _ptr(hit_off), _ptr(out["target"]), _ptr(out["score"]), _ptr(out["end_j"]),
                                               _ptr(out["strand"]), _ptr(stats), _ptr(ncigar), _ptr(cigar_off), _ptr(words),
                                               cap if cigar else 0))
            n = int(hit_off[nq])
            if n > hit_cap:
                hit_cap = n
                continue
            if not cigar or cigar_off[n] <= cap:
                break
            cap = int(cigar_off[n])
        res = {name: a[:n].copy() for name, a in out.items()}
        res["hit_off"] = hit_off
        if cigar:
            res["stats"], res["ncigar"], res["cigar_off"] = stats[:n].copy(), ncigar[:n].copy(), cigar_off[:n + 1].copy()
            res["cigar"] = [words[cigar_off[e]:cigar_off[e] + max(int(ncigar[e]), 0)].copy() for e in range(n)]
        return res

    def allpairs_hits(self, mode, reads, threshold, first_pair=0, npairs=None, cigar=False, cigar_m=False, chunk_pairs=0):
        """All-vs-all over `reads` (a list of str or bytes) of which only the pairs over a threshold come back (at_allpairs_hits): the
        pairs (a < b) of the triangle's range [first_pair, first_pair + npairs) -- npairs None: to its end -- whose score is >=
        threshold (edit: whose distance is <= threshold), in ascending pair order.  Returns a dict: pair (int64, the triangle index)
        and a, b, score, end_i, end_j, state (int32) over the hits, exactly what align_allpairs_stream gives for those pairs; with
        cigar=True (not for edit) also stats (nhits, 8), ncigar (nhits,), cigar_off (nhits + 1,) and cigar, a list of numpy uint32
        arrays ('=' / 'X'; cigar_m: 'M').  With "overlap" the pairs the bit-parallel bound proves below the threshold are not swept;
        the handle's set_min_score setting is the same afterwards.  chunk_pairs (pairs per slice; 0: the default) does not change
        the results."""
        if isinstance(mode, str):
            mode = MODES[mode]
        rs = [_b(x) for x in reads]
        n = len(rs)
        lens = np.fromiter((len(x) for x in rs), dtype=np.int32, count=n)
        off = np.zeros(n, dtype=np.int64)
        if n > 1:
            np.cumsum(lens[:-1], out=off[1:])
        blob = np.frombuffer(b"".join(rs) + b"\0", dtype=np.uint8).copy()
        if npairs is None:
            npairs = n * (n - 1) // 2 - int(first_pair)
        nhits = C.c_int64(0)
        hit_cap, cap = 4 * n + 1024, 0
        for _ in range(3):                                      # more hits, then more runs, than the first guess has room for
            pair = np.zeros(hit_cap, dtype=np.int64)
            out = {name: np.zeros(hit_cap, dtype=np.int32) for name in ("a", "b", "score", "end_i", "end_j", "state")}
            stats = np.full((hit_cap, 8), -1, dtype=np.int32) if cigar else None
            ncigar = np.zeros(hit_cap, dtype=np.int32) if cigar else None
            cigar_off = np.zeros(hit_cap + 1, dtype=np.int64) if cigar else None
            cap = max(cap, 16 * hit_cap + 64)
            words = np.zeros(cap, dtype=np.uint32) if cigar else None
            self._check(self._lib.at_allpairs_hits(self._h, mode, n, _ptr(blob), _ptr(off), _ptr(lens), int(first_pair), int(npairs),
                                                   int(threshold), int(chunk_pairs), CIGAR_M if cigar_m else 0, hit_cap, C.addressof(nhits),
                                                   _ptr(pair), _ptr(out["a"]), _ptr(out["b"]), _ptr(out["score"]), _ptr(out["end_i"]),
                                                   _ptr(out["end_j"]), _ptr(out["state"]), _ptr(stats), _ptr(ncigar), _ptr(cigar_off),
                                                   _ptr(words), cap if cigar else 0))
            k = int(nhits.value)
            if k > hit_cap:
                hit_cap = k
                continue
            if not cigar or cigar_off[k] <= cap:
                break
            cap = int(cigar_off[k])
        res = {name: a[:k].copy() for name, a in out.items()}
        res["pair"] = pair[:k].copy()
        if cigar:
            res["stats"], res["ncigar"], res["cigar_off"] = stats[:k].copy(), ncigar[:k].copy(), cigar_off[:k + 1].copy()
            res["cigar"] = [words[cigar_off[e]:cigar_off[e] + max(int(ncigar[e]), 0)].copy() for e in range(k)]
        return res

    def align_allpairs_device(self, mode, nreads, d_seq, bits, d_woff, d_len, max_len, first_pair, npairs, want_traceback,
                              d_score, d_end_i, d_end_j, d_state, d_ops, d_ops_off, d_nops, stream=0):
        """All ordered pairs (a < b) of one read set; see at_align_allpairs_device in include/aligntools_hip.h."""
        self._check(self._lib.at_align_allpairs_device(self._h, mode, nreads, d_seq, bits, d_woff, d_len, max_len, first_pair,
                                                       npairs, 1 if want_traceback else 0, d_score, d_end_i, d_end_j, d_state,
                                                       d_ops, d_ops_off, d_nops, stream))


_default = None


def default_aligner():
    global _default
    if _default is None:
        _default = Aligner()
    return _default


def _single(mode, s1, s2, opt):
    al = default_aligner()
    al.set_opt(opt)
    r = al.align_batch(mode, [(s1, s2)])
    if mode == MODE_EDIT:
        return int(r["score"][0])
    return float(r["score"][0]), r["r1"][0], r["r2"][0]


# ---- the reference's five kernels, same names and argument meaning (opt_t) ----
def align_gla(s1, s2, opt=None):
    """Global affine alignment (reference alignment.h:417).  Returns (score, r1, r2)."""
    return _single(MODE_GLOBAL, s1, s2, opt or opt_t())


def align_local_affine(s1, s2, opt=None):
    """Smith-Waterman affine (reference alignment.h:805).  Returns (score, r1, r2)."""
    return _single(MODE_LOCAL, s1, s2, opt or opt_t())


def align_fit_affine_jump(s1, s2, opt=None):
    """Fit alignment, jump state when opt.s (reference alignment.h:596).  Raises
    like the reference dies when s1 is longer than s2 (:599)."""
    return _single(MODE_FIT, s1, s2, opt or opt_t())


def align_overlap(s1, s2, opt=None):
    """Overlap alignment, linear gap (reference alignment.h:926)."""
    return _single(MODE_OVERLAP, s1, s2, opt or opt_t())


def edit_dist(s1, s2, opt=None):
    """Edit distance with `-u` as the signed mismatch cost (reference alignment.h:291)."""
    return _single(MODE_EDIT, s1, s2, opt or opt_t())
