"""Environment knobs against the oracle.

The rule: under any setting of any knob, a call either returns results equal to the oracle for every pair, or refuses with a
nonzero code and an error text.  It never returns AT_OK with wrong results.

  * the CPU half (no mark): every knob the library reads (getenv / env_* literals in aligntools/c_amd/csrc and host/) is in KNOBS
    below -- with the test that sets it, or a one-line reason why it cannot change a result -- and in DESIGN.md section 7's table;
  * the GPU half (-m gpu): allocation failures forced through AT_DIAG_FAIL_ALLOC, the knobs no other test sets, and batches shrunk
    onto a few waves so that every wave works through several items.  Every pair of every batch is checked against the oracle
    (oracle/at_oracle.c, run on a pool of threads: ctypes releases the GIL and the restatement keeps no shared state).
"""
import ctypes as C
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOMEM = -6

# knob -> the test that sets it ("path::name"), or "reason: ..." why it cannot change a result
KNOBS = {
    "AT_GROUP": "tests/test_gpu_parity.py::test_packed_32_lane_groups",
    "AT_TWO_PASS": "tests/test_gpu_parity.py::test_two_pass_tracebacks",
    "AT_TP_SPLIT": "tests/test_gpu_parity.py::test_two_pass_tracebacks",
    "AT_WALK_TEAMS": "tests/test_gpu_parity.py::test_two_pass_walk_kernel_batches",
    "AT_CK_PIECE_PAIRS": "tests/test_gpu_parity.py::test_two_pass_walk_kernel_batches",
    "AT_TAIL_SPLIT": "tests/test_gpu_parity.py::test_sliver_of_a_batch_on_64_lane_groups",
    "AT_HOST_CHUNKS": "tests/test_gpu_parity.py::test_chunked_host_entry",
    "AT_MYERS_LANE_MIN_PAIRS": "tests/test_gpu_parity.py::test_bit_parallel_edit_distance",
    "AT_NO_PACKED": "tests/test_default_routing.py::test_batches_on_both_sides_of_the_packed_threshold",
    "AT_PACKED_MIN_ROUNDS": "tests/test_default_routing.py::test_batches_on_both_sides_of_the_packed_threshold",
    "AT_QUIET_FIT": "tests/test_boundary_proof.py::test_reference_drivers_link_against_the_boundary",
    "AT_CLI_CHUNK": "tests/test_cli.py::test_cli_batch_streams_chunks_and_scales_all_vs_all",
    "AT_CLI_FIRST_CHUNK": "tests/test_cli.py::test_cli_batch_streams_chunks_and_scales_all_vs_all",
    "AT_RCCL_LIB": "tests/test_cli.py::test_cli_batch_gpus_n_matches_one_gpu",
    "AT_ONE_DEVICE": "tests/test_cli.py::test_cli_batch_gpus_n_matches_one_gpu",
    "AT_COMM_FORCE_RCCL": "tests/test_cli.py::test_cli_batch_gpus_n_matches_one_gpu",
    "AT_RANK": "tests/test_cli.py::test_cli_batch_gpus_n_matches_one_gpu",
    "AT_WORLD": "tests/test_cli.py::test_cli_batch_gpus_n_matches_one_gpu",
    "AT_COMM_DIR": "tests/test_cli.py::test_cli_batch_gpus_n_matches_one_gpu",
    "AT_DEVICE": "reason: the card the C host binds to (the --gpus N launcher sets it per rank); no kernel or result depends on it",
    "AT_CLI_CHUNK_BASES": "reason: a second bound, in bases, on the CLI's chunks -- the same cut AT_CLI_CHUNK makes in the test named for it",
    "AT_FAST_EXIT": "reason: how the CLI process ends, after its output is flushed",
    "AT_HOST_TRACE": "reason: time stamps on stderr only",
    "AT_CLI_TRACE": "reason: time stamps on stderr only",
    # this module
    "AT_DIAG_FAIL_ALLOC": "tests/test_knobs.py::test_checkpoint_allocation_failure_falls_back",
    "AT_CK_CAP_MB": "tests/test_knobs.py::test_checkpoint_cap_below_one_work_item",
    "AT_DIAG_NO_WALK_KERNEL": "tests/test_knobs.py::test_product_ignores_the_sweep_only_knob",
    "AT_STORE": "tests/test_knobs.py::test_int32_storage_classes",
    "AT_ROWS_PER_LANE": "tests/test_knobs.py::test_int32_rows_per_lane",
    "AT_SMALL_LDS_LIMIT": "tests/test_knobs.py::test_storage_class_thresholds",
    "AT_MEDIUM_LDS_LIMIT": "tests/test_knobs.py::test_storage_class_thresholds",
    "AT_WAVES_PER_CU": "tests/test_knobs.py::test_many_items_per_wave",
    "AT_WS_CAP_MB": "tests/test_knobs.py::test_many_items_per_wave",
    "AT_WALK_WAVES_PER_CU": "tests/test_knobs.py::test_persistent_walkers",
    "AT_TP_RESERVE": "tests/test_knobs.py::test_persistent_walkers",
    "AT_AUTO_UNIFORM": "tests/test_knobs.py::test_device_entry_auto_uniform",
    "AT_RAGGED_PACKED": "tests/test_knobs.py::test_routing_knobs",
    "AT_RAGGED_MIN_BUCKET": "tests/test_knobs.py::test_routing_knobs",
    "AT_NO_PACKED_OVERLAP": "tests/test_knobs.py::test_routing_knobs",
    "AT_MYERS": "tests/test_knobs.py::test_routing_knobs",
    "AT_MYERS_GROUP": "tests/test_knobs.py::test_routing_knobs",
    "AT_MYERS_LANE_MAX": "tests/test_knobs.py::test_routing_knobs",
    "AT_OVERLAP_FILTER": "tests/test_knobs.py::test_all_vs_all_knobs",
    "AT_ALLPAIRS_CHUNK": "tests/test_knobs.py::test_all_vs_all_knobs",
    "AT_HOST_PACK": "tests/test_knobs.py::test_host_entry_knobs",
    "AT_HOST_STAGE_PIECE": "tests/test_knobs.py::test_host_entry_knobs",
    "AT_HOST_NO_PINNED_CALLER": "tests/test_knobs.py::test_host_entry_knobs",
    "AT_HOST_CHUNK_MIN": "tests/test_knobs.py::test_host_entry_knobs",
    "AT_RENDER_GROUP": "tests/test_knobs.py::test_host_entry_knobs",
}


def _library_knobs():
    pat = re.compile(r'\b(?:getenv|secure_getenv|env_[a-z0-9_]+)\s*\(\s*"(AT_[A-Z0-9_]+)"')
    names = set()
    for sub in ("csrc", "host"):
        d = os.path.join(ROOT, "aligntools", "c_amd", sub)
        for f in sorted(os.listdir(d)):
            with open(os.path.join(d, f), errors="replace") as fh:
                names.update(pat.findall(fh.read()))
    return names


def test_every_knob_has_a_test_or_a_reason():
    names = _library_knobs()
    assert len(names) > 30, sorted(names)
    missing = sorted(names - set(KNOBS))
    assert not missing, "knobs the library reads without an entry in tests/test_knobs.py KNOBS: %s" % missing
    stale = sorted(set(KNOBS) - names)
    assert not stale, "KNOBS entries the library no longer reads: %s" % stale
    for name, what in KNOBS.items():
        if what.startswith("reason: "):
            assert len(what) > 20, name
            continue
        path, test = what.split("::")
        with open(os.path.join(ROOT, path)) as fh:
            assert re.search(r"^def %s\(" % re.escape(test), fh.read(), re.M), (name, what)


def test_every_knob_is_in_the_design_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    sec = text[text.index("## 7. Notes"):]
    table = "\n".join(line for line in sec.splitlines() if line.startswith("  |"))
    missing = sorted(n for n in _library_knobs() if not re.search(r"`%s`" % n, table) and not re.search(r"\b%s\b" % n, table))
    assert not missing, "knobs missing from DESIGN.md section 7's table: %s" % missing


# ---------------------------------------------------------------- GPU half

@pytest.fixture(scope="module")
def al():
    import aligntools.c_amd as A
    before = os.environ.get("AT_PACKED_MIN_ROUNDS")
    os.environ["AT_PACKED_MIN_ROUNDS"] = "0"   # small test batches must still reach the 64-lane packed kernels
    a = A.Aligner()
    yield a
    a.close()
    if before is None:
        os.environ.pop("AT_PACKED_MIN_ROUNDS", None)
    else:
        os.environ["AT_PACKED_MIN_ROUNDS"] = before


@pytest.fixture
def env(monkeypatch):
    """monkeypatch with one chunk per host-entry call (a chunk on a helper handle would keep its own last_config)"""
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    return monkeypatch


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _mk(rng, l1, l2, alpha="ACGT"):
    """a pair of exactly l1 x l2 bases: unrelated, or s2 a noisy copy of s1 between random flanks"""
    a = "".join(rng.choice(alpha) for _ in range(l1))
    if rng.random() < 0.4:
        return a, "".join(rng.choice(alpha) for _ in range(l2))
    t = list(a)
    for _ in range(1 + l1 // 12):
        q = rng.randrange(len(t))
        r = rng.random()
        if r < 0.5:
            t[q] = rng.choice(alpha)
        elif r < 0.75 and len(t) > 1:
            del t[q]
        else:
            t.insert(q, rng.choice(alpha))
    pre = "".join(rng.choice(alpha) for _ in range(rng.randint(0, max(0, l2 - l1))))
    post = "".join(rng.choice(alpha) for _ in range(l2))
    return a, (pre + "".join(t) + post)[:l2]


def _batch(rng, n, r1, r2, fit=False, alpha="ACGT"):
    """n pairs, l1 in r1 and l2 in r2 (inclusive ranges; equal ends: a uniform batch); fit: l2 >= l1"""
    out = []
    for _ in range(n):
        l1 = rng.randint(*r1)
        l2 = rng.randint(*r2)
        if fit:
            l2 = max(l1, l2)
        out.append(_mk(rng, l1, l2, alpha))
    return out


def _oracle(mode, pairs, sc, uj, sites):
    """the restatement's result for every distinct pair, on at most 16 threads"""
    uniq = list(dict.fromkeys(pairs))
    O.align(O.MODE_NAMES[mode], "A", "A")           # (loads the library before the threads start)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda p: O.align(O.MODE_NAMES[mode], p[0], p[1], *sc, uj, sites), uniq))
    return dict(zip(uniq, res))


def _compare(res, mode, pairs, sc, uj, sites, tb, ctx):
    ref = _oracle(mode, pairs, sc, uj, sites)
    for k, p in enumerate(pairs):
        r = ref[p]
        assert r["rc"] == 0, (ctx, k)
        assert int(res["score"][k]) == r["score"], (ctx, k, p[0][:30], p[1][:30])
        if mode == "edit":
            continue
        assert (int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k])) == (r["end_i"], r["end_j"], r["state"]), (ctx, k)
        if tb:
            assert res["ops"][k] == r["ops"], (ctx, k)


SC = (2, -2, -5, -1, -10)


def _run(al, mode, pairs, sc=SC, tb=True, sites=None, ctx=""):
    """align_batch + every pair against the oracle; mode "fitj" = fit with the jump state.  Returns last_config."""
    uj = mode == "fitj"
    mode = "fit" if uj else mode
    sites = list(sites if sites is not None else ([7, 50, 51, 120, 300] if uj else []))
    al.set_scoring(*sc, uj, sites)
    res = al.align_batch(mode, pairs, traceback=tb, render=False)
    cfg = al.last_config
    _compare(res, mode, pairs, sc, uj, sites, tb and mode != "edit", (ctx, mode, cfg))
    return cfg


def _grid(cfg):
    return int(re.search(r"grid=(\d+)", cfg).group(1))


def _hip_last_error():
    import aligntools.c_amd as A
    fn = A.load_library().hipPeekAtLastError     # (the runtime the shim is linked against, through its handle)
    fn.restype = C.c_int
    return fn()


# ---- A: allocation failures

C3 = ("global", 1024, 1024, (1, -1, -4, -1, -10), [])
C4 = ("fitj", 150, 500, (2, -2, -5, -1, -10), [100, 200, 300, 400])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["C3", "C4"])
def test_checkpoint_allocation_failure_falls_back(al, env, shape):
    """AT_DIAG_FAIL_ALLOC=ck: the checkpoint buffer of the walk kernel cannot be allocated (the runtime really refuses 2^50 bytes).
    C3's shape (64-lane groups) falls back to the two-pass rounds inside the sweep's kernel, C4's (8-lane groups) to the one-pass
    kernels: AT_OK, every pair equal to the oracle, last_config says so, no hipMalloc text in at_last_error, no error left in the
    caller's thread.  The handle keeps to the fallback; a new handle takes the walk kernel again."""
    import aligntools.c_amd as A
    mode, l1, l2, sc, sites = C3 if shape == "C3" else C4
    rng = random.Random(l1 + l2)
    n = 61 if shape == "C3" else 403
    pairs = _batch(rng, n, (l1, l1), (l2, l2))
    h = A.Aligner()
    try:
        env.setenv("AT_DIAG_FAIL_ALLOC", "ck")
        cfg = _run(h, mode, pairs, sc, sites=sites, ctx=shape)
        assert "walk kernel" not in cfg and "checkpoint buffer unavailable" in cfg, cfg
        assert ("two-pass" in cfg) == (shape == "C3"), cfg
        assert "hipMalloc" not in h._lib.at_last_error(h._h).decode()
        assert _hip_last_error() == 0
        env.delenv("AT_DIAG_FAIL_ALLOC")
        pairs2 = _batch(rng, n - 8, (l1, l1), (l2, l2))
        cfg = _run(h, mode, pairs2, sc, sites=sites, ctx=shape + " second batch")
        assert "walk kernel" not in cfg and "checkpoint buffer unavailable" in cfg, cfg
    finally:
        h.close()
    cfg = _run(al, mode, pairs[:40], sc, sites=sites, ctx=shape + " other handle")
    assert "walk kernel" in cfg and "checkpoint" not in cfg, cfg


@pytest.mark.gpu
def test_workspace_allocation_failure_refuses_then_recovers(al, env):
    """AT_DIAG_FAIL_ALLOC=ws: the pointer slots cannot be allocated -- AT_ERR_NOMEM with the runtime's text, and nothing left in the
    thread's last error: the next call on the same handle and on another one return AT_OK with correct results."""
    import aligntools.c_amd as A
    rng = random.Random(11)
    pairs = _batch(rng, 100, (150, 150), (150, 150))
    h = A.Aligner()
    try:
        h.set_scoring(*SC, False, [])
        env.setenv("AT_DIAG_FAIL_ALLOC", "ws")
        with pytest.raises(A.AlignToolsError) as ei:
            h.align_batch("local", pairs)
        assert ei.value.code == NOMEM and "hipMalloc" in str(ei.value), ei.value
        assert _hip_last_error() == 0
        env.delenv("AT_DIAG_FAIL_ALLOC")
        cfg = _run(h, "local", pairs, ctx="same handle")
        assert "hbm-pointers" in cfg, cfg
        cfg = _run(al, "local", pairs[:50], ctx="other handle")
        assert "hbm-pointers" in cfg, cfg
    finally:
        h.close()


@pytest.mark.gpu
def test_stale_error_of_the_caller_is_not_the_calls(al, env):
    """An allocation the caller's thread saw fail just before (the runtime's last error still set) does not fail the next batch."""
    import aligntools.c_amd as A
    lib = A.load_library()
    p = C.c_void_p()
    lib.hipMalloc.restype = C.c_int
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    assert lib.hipMalloc(C.byref(p), 1 << 50) != 0
    rng = random.Random(12)
    _run(al, "global", _batch(rng, 40, (20, 200), (20, 260)), ctx="after a failed hipMalloc of the caller's")


@pytest.mark.gpu
def test_checkpoint_cap_below_one_work_item(al, env):
    """AT_CK_CAP_MB=1 below one work item's checkpoints (C3's kernel against a second sequence of 3 000 bases: ~2.8 MB per item): the
    batch takes the rounds inside the sweep's kernel instead of failing; without the cap the same handle takes the walk kernel again."""
    mode, l1, l2, sc = "global", 1000, 3000, C3[3]
    rng = random.Random(13)
    pairs = _batch(rng, 45, (l1, l1), (l2, l2))
    env.setenv("AT_CK_CAP_MB", "1")
    cfg = _run(al, mode, pairs, sc, ctx="cap 1 MB")
    assert "two-pass" in cfg and "walk kernel" not in cfg and "exceed AT_CK_CAP_MB" in cfg, cfg
    env.delenv("AT_CK_CAP_MB")
    cfg = _run(al, mode, pairs[:20], sc, ctx="no cap")
    assert "walk kernel" in cfg and "AT_CK_CAP_MB" not in cfg, cfg


@pytest.mark.gpu
def test_product_ignores_the_sweep_only_knob(al, env):
    """AT_DIAG_NO_WALK_KERNEL=1 skips pass 2 only in diagnostic builds (-DAT_DIAG_SWEEP_ONLY=1); the product runs the walk kernel."""
    mode, l1, l2, sc, sites = C4
    env.setenv("AT_DIAG_NO_WALK_KERNEL", "1")
    cfg = _run(al, mode, _batch(random.Random(14), 77, (l1, l1), (l2, l2)), sc, sites=sites)
    assert "walk kernel" in cfg, cfg


# ---- B: knob matrix

MODES6 = ["global", "local", "fit", "fitj", "overlap", "edit"]
STORE_NAMES = {0: "store=lds ", 1: "store=lds+hbm-pointers ", 2: "store=hbm "}


@pytest.mark.gpu
@pytest.mark.parametrize("store", [0, 1, 2])
def test_int32_storage_classes(al, env, store):
    """AT_STORE on the int32 kernels: every mode, with and without tracebacks, 2-bit and byte words.  Scores only there is no pointer
    matrix, so store 1 is store 0 (choose_store)."""
    env.setenv("AT_NO_PACKED", "1")
    env.setenv("AT_STORE", str(store))
    rng = random.Random(20 + store)
    for mode in MODES6:
        for tb in (True, False):
            for alpha in ("ACGT", "ACGTN"):
                pairs = _batch(rng, 37, (1, 200), (1, 300), fit=mode.startswith("fit"), alpha=alpha)
                cfg = _run(al, mode, pairs, (1, -2, -5, -1, -10), tb=tb, ctx=(store, tb, alpha))
                assert cfg.startswith("int32"), cfg
                want = store if (tb and mode != "edit") or store != 1 else 0
                assert STORE_NAMES[want] in cfg, (mode, tb, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("store", [0, 1, 2])
def test_packed_64_lane_storage_classes(al, env, store):
    """AT_STORE on the packed 64-lane group (AT_GROUP=64, one-pass tracebacks).  The group has an instantiation for every storage
    class and 1..4 rows per lane (at_k16_g64.hip), and these shapes fit LDS at store 0: no fallback, no refusal."""
    env.setenv("AT_GROUP", "64")
    env.setenv("AT_TWO_PASS", "0")
    env.setenv("AT_STORE", str(store))
    rng = random.Random(30 + store)
    for mode, l1, l2 in (("global", 200, 240), ("local", 90, 90), ("fitj", 120, 300)):
        cfg = _run(al, mode, _batch(rng, 33, (l1, l1), (l2, l2)), ctx=store)
        assert STORE_NAMES[store] in cfg and "1x64-lane groups" in cfg, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_int32_rows_per_lane(al, env, k):
    """AT_ROWS_PER_LANE=1..4 on the int32 kernels: reads cut into up to five strips of 64 k rows."""
    env.setenv("AT_NO_PACKED", "1")
    env.setenv("AT_ROWS_PER_LANE", str(k))
    rng = random.Random(40 + k)
    for mode, tb in (("global", True), ("local", True), ("fitj", True), ("overlap", True), ("local", False)):
        cfg = _run(al, mode, _batch(rng, 31, (1, 300), (1, 320), fit=mode == "fitj"), tb=tb, ctx=k)
        assert cfg.startswith("int32") and "rows/lane=%d " % k in cfg, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 16])
def test_int32_deep_rows_per_lane(al, env, k):
    """AT_ROWS_PER_LANE=8 / 16: the one-state kernels without a pointer matrix (overlap scores, edit on the cell-by-cell kernel)."""
    env.setenv("AT_ROWS_PER_LANE", str(k))
    env.setenv("AT_MYERS", "0")
    rng = random.Random(50 + k)
    for mode, sc in (("overlap", SC), ("edit", (1, -2, -5, -1, -10)), ("edit", (1, 1, -5, -1, -10))):
        cfg = _run(al, mode, _batch(rng, 29, (1, 1100), (1, 700)), sc, tb=False, ctx=k)
        assert cfg.startswith("int32") and "rows/lane=%d " % k in cfg, cfg


@pytest.mark.gpu
def test_storage_class_thresholds(al, env):
    """AT_SMALL_LDS_LIMIT / AT_MEDIUM_LDS_LIMIT move the int32 kernels between the three storage classes."""
    env.setenv("AT_NO_PACKED", "1")
    rng = random.Random(60)
    small = _batch(rng, 40, (1, 60), (1, 80))
    large = _batch(rng, 40, (150, 200), (200, 300))
    cfg = _run(al, "global", small, ctx="default small")
    assert "store=lds " in cfg, cfg
    cfg = _run(al, "global", large, ctx="default large")
    assert "store=lds+hbm-pointers " in cfg, cfg
    env.setenv("AT_SMALL_LDS_LIMIT", "0")
    cfg = _run(al, "local", small, ctx="small limit 0")
    assert "store=lds+hbm-pointers " in cfg, cfg
    env.setenv("AT_MEDIUM_LDS_LIMIT", "0")
    cfg = _run(al, "fitj", _batch(rng, 40, (1, 60), (60, 80)), ctx="both limits 0")
    assert "store=hbm " in cfg, cfg
    env.setenv("AT_SMALL_LDS_LIMIT", str(150 * 1024))
    env.delenv("AT_MEDIUM_LDS_LIMIT")
    cfg = _run(al, "global", large, ctx="small limit 150 KB")
    assert "store=lds " in cfg, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    # width, AT_WALK_WAVES_PER_CU, AT_CK_PIECE_PAIRS and pairs (in units of n x CUs x 128 alignments), AT_TP_RESERVE, AT_TAIL_SPLIT
    ("C4", 1, 0, 1.3, 0, 0),
    ("C4", 2, 0, 1.2, 2, 0),
    ("C4", 1, 1.3, 2.5, 0, 0),     # two pieces, the last 1.2 units: the walkers of each piece refill
    ("C4", 1, 0, None, 0, 1),      # two whole rounds of the sweep's grid and a sliver on 32-lane items (whose walkers are not capped)
    ("C3", 1, 0, 1.3, 0, 1),       # 64-lane groups x 16 rows without teams (AT_WALK_TEAMS=0): one walker per half-lane
    ("C3", 2, 0, 1.2, 0, 1),
])
def test_persistent_walkers(al, env, case):
    """AT_WALK_WAVES_PER_CU=n: at most n walker wavefronts per CU, which refill from the counters behind the sweep's work counter.
    Every launch (every piece) has more main alignments than its walkers' first round takes, 128 per wavefront -- at_last_config
    names the walkers of the first and the last piece -- so that walkers take further alignments (C4: the jump state; with pieces,
    whose counters are zeroed per piece).  AT_TP_RESERVE leaves wave slots of the sweep free.  Every pair against the oracle (a few
    hundred distinct pairs, repeated with a prime period)."""
    width, wcap, piece, units, rsv, tail = case
    mode, l1, l2, sc, sites = C4 if width == "C4" else ("global", 609, 120, (1, -1, -4, -1, -10), [])   # (C3's kernel, a short s2)
    ncu = _ncu()
    unit = wcap * ncu * 128
    rng = random.Random(70 + wcap)
    if units is None:
        # the sweep's grid G from a probe; then 2 G items and G / 8 + 1 more: the last round less than a quarter full
        al.set_scoring(*sc, True, sites)
        al.align_batch("fit", _batch(rng, 40, (l1, l1), (l2, l2)), render=False)
        g = int(re.search(r"waves/cu<=(\d+)", al.last_config).group(1)) * ncu
        n = 16 * (2 * g + g // 8) + 5
    else:
        n = int(units * unit) + 37
    uniq = _batch(rng, 397 if width == "C4" else 211, (l1, l1), (l2, l2))
    pairs = [uniq[k % len(uniq)] for k in range(n)]
    env.setenv("AT_WALK_WAVES_PER_CU", str(wcap))
    env.setenv("AT_TAIL_SPLIT", str(tail))
    if width == "C3":
        env.setenv("AT_WALK_TEAMS", "0")
    if piece:
        env.setenv("AT_CK_PIECE_PAIRS", str(int(piece * unit)))
    if rsv:
        env.setenv("AT_TP_RESERVE", str(rsv))
    cfg = _run(al, mode, pairs, sc, sites=sites, ctx=case)
    assert "walk kernel" in cfg, cfg
    walkers = [(int(w), int(a)) for w, a in re.findall(r"\[walkers: (\d+) wavefronts for (\d+) alignments\]", cfg)]
    assert len(walkers) == (2 if piece else 1), cfg
    for w, a in walkers:
        assert w == wcap * ncu and w * 128 < a, (case, cfg)
    if piece:
        assert "in pieces of" in cfg, cfg
    if rsv:
        assert "AT_TP_RESERVE: sweep grid=" in cfg, cfg
    if tail:
        assert width != "C4" or "as 32-lane items" in cfg, cfg


@pytest.mark.gpu
def test_device_entry_auto_uniform(al, env):
    """AT_AUTO_UNIFORM=0: the device entry without the uniform promise no longer lets the device check the shapes (int32 kernel)."""
    import torch
    import aligntools.c_amd as A
    rng = random.Random(80)
    pairs = _batch(rng, 4099, (100, 100), (120, 120))
    words, woff1, woff2, len1, len2, bits = A.pack_pairs([(a.encode(), b.encode()) for a, b in pairs])
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("w", words.view(np.int32)), ("o1", woff1), ("o2", woff2), ("l1", len1), ("l2", len2))}
    n = len(pairs)
    ref = _oracle("global", pairs, SC, False, [])
    al.set_scoring(*SC, False, [])
    for auto in ("1", "0"):
        env.setenv("AT_AUTO_UNIFORM", auto)
        out = torch.full((5, n), -7, dtype=torch.int32, device=dev)
        ops = torch.zeros(n * 220 + 64, dtype=torch.uint8, device=dev)
        ops_off = torch.arange(n, dtype=torch.int64, device=dev) * 220
        stream = torch.cuda.current_stream().cuda_stream
        al.align_batch_device(A.MODES["global"], n, d["w"].data_ptr(), bits, d["o1"].data_ptr(), d["l1"].data_ptr(), d["o2"].data_ptr(),
                              d["l2"].data_ptr(), 100, 120, False, True, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                              out[3].data_ptr(), ops.data_ptr(), ops_off.data_ptr(), out[4].data_ptr(), stream)
        torch.cuda.synchronize()
        cfg = al.last_config
        assert cfg.startswith("auto:") == (auto == "1"), cfg
        o = out.cpu().numpy()
        h_ops = ops.cpu().numpy()
        for k, p in enumerate(pairs):
            r = ref[p]
            assert (int(o[0][k]), int(o[1][k]), int(o[2][k]), int(o[3][k])) == (r["score"], r["end_i"], r["end_j"], r["state"]), (auto, k)
            assert bytes(h_ops[k * 220:k * 220 + o[4][k]]) == r["ops"], (auto, k)


@pytest.mark.gpu
def test_routing_knobs(al, env):
    """One batch per routing knob, at sizes where it takes effect."""
    rng = random.Random(90)
    ragged = _batch(rng, 300, (30, 150), (30, 160))
    cfg = _run(al, "local", ragged, ctx="ragged, default")
    assert "frames" in cfg, cfg
    frames_default = int(re.search(r"\((\d+) frames", cfg).group(1))
    env.setenv("AT_RAGGED_MIN_BUCKET", "16")
    cfg = _run(al, "local", ragged, ctx="AT_RAGGED_MIN_BUCKET=16")
    assert int(re.search(r"\((\d+) frames", cfg).group(1)) > frames_default, cfg
    env.delenv("AT_RAGGED_MIN_BUCKET")
    env.setenv("AT_RAGGED_PACKED", "0")
    cfg = _run(al, "global", ragged, ctx="AT_RAGGED_PACKED=0")
    assert cfg.startswith("int32") and "frames" not in cfg, cfg
    env.delenv("AT_RAGGED_PACKED")
    ovl = _batch(rng, 50, (140, 140), (150, 150))
    cfg = _run(al, "overlap", ovl, ctx="overlap, default")
    assert cfg.startswith("packed16"), cfg
    env.setenv("AT_NO_PACKED_OVERLAP", "1")
    cfg = _run(al, "overlap", ovl, ctx="AT_NO_PACKED_OVERLAP=1")
    assert cfg.startswith("int32"), cfg
    edit = _batch(rng, 70, (1, 200), (1, 250))
    unit = (1, 1, -5, -1, -10)
    cfg = _run(al, "edit", edit, unit, tb=False, ctx="edit, default")
    assert "myers" in cfg and "x1-lane groups" in cfg, cfg
    env.setenv("AT_MYERS_GROUP", "8")
    cfg = _run(al, "edit", edit, unit, tb=False, ctx="AT_MYERS_GROUP=8")
    assert "myers" in cfg and "8x8-lane groups" in cfg, cfg
    env.delenv("AT_MYERS_GROUP")
    env.setenv("AT_MYERS_LANE_MAX", "100")
    cfg = _run(al, "edit", edit, unit, tb=False, ctx="AT_MYERS_LANE_MAX=100")
    assert "myers" in cfg and "8x8-lane groups" in cfg, cfg
    env.setenv("AT_MYERS", "0")
    cfg = _run(al, "edit", edit, unit, tb=False, ctx="AT_MYERS=0")
    assert cfg.startswith("int32"), cfg


@pytest.mark.gpu
def test_all_vs_all_knobs(al, env):
    """AT_OVERLAP_FILTER=0: a threshold no longer stops any pair (every pair exact); AT_ALLPAIRS_CHUNK: slices of that many pairs."""
    import aligntools.c_amd as A
    rng = random.Random(100)
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(50, 300))) for _ in range(45)]
    for k in range(0, 44, 3):
        reads[k + 1] = (reads[k][-60:] + reads[k + 1])[:300]
    blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    nr = len(reads)
    total = nr * (nr - 1) // 2
    pairs = [(reads[a], reads[b]) for a in range(nr) for b in range(a + 1, nr)]
    ref = _oracle("overlap", pairs, SC, False, [])
    al.set_scoring(*SC, False, [])

    def sweep():
        got = np.full((4, total), -7, dtype=np.int64)

        def on_slice(first, sc, ei, ej, st):
            for row, x in enumerate((sc, ei, ej, st)):
                got[row, first:first + len(x)] = x
        al.align_allpairs_stream("overlap", blob, off, lens, 0, total, 0, on_slice)
        return got

    try:
        al.set_min_score(40)
        env.setenv("AT_OVERLAP_FILTER", "0")
        env.setenv("AT_ALLPAIRS_CHUNK", "97")
        got = sweep()
        cfg = al.last_config
        assert "filter" not in cfg and "slices of <= 97 pairs" in cfg, cfg
    finally:
        al.set_min_score(None)
    for t, p in enumerate(pairs):
        r = ref[p]
        assert (got[0][t], got[1][t], got[2][t], got[3][t]) == (r["score"], r["end_i"], r["end_j"], r["state"]), t


@pytest.mark.gpu
def test_host_entry_knobs(al, env):
    """The host entry's upload paths (AT_HOST_PACK, AT_HOST_STAGE_PIECE, AT_HOST_NO_PINNED_CALLER with a page-locked blob), its chunks
    (AT_HOST_CHUNK_MIN) and the rendering kernel's group width (AT_RENDER_GROUP), each with every pair against the oracle."""
    import torch
    import aligntools.c_amd as A
    rng = random.Random(110)
    pairs = _batch(rng, 200, (100, 300), (100, 320))
    cfg = _run(al, "global", pairs, ctx="default upload")
    assert "[upload: 2-bit words packed on the host, 1 pieces]" in cfg, cfg
    env.setenv("AT_HOST_STAGE_PIECE", "4096")
    cfg = _run(al, "global", pairs, ctx="host packing in pieces")
    assert int(re.search(r"packed on the host, (\d+) pieces", cfg).group(1)) >= 8, cfg
    env.setenv("AT_HOST_PACK", "0")
    cfg = _run(al, "local", pairs, ctx="raw bytes in pieces")
    assert int(re.search(r"raw bytes staged, (\d+) pieces", cfg).group(1)) >= 10, cfg
    env.delenv("AT_HOST_STAGE_PIECE")
    env.delenv("AT_HOST_PACK")
    # a caller's page-locked blob: copied from in place, or staged all the same with AT_HOST_NO_PINNED_CALLER=1
    blob, off1, len1, off2, len2 = A._flatten([(a.encode(), b.encode()) for a, b in pairs])
    pinned = torch.from_numpy(blob).pin_memory()
    n = len(pairs)
    al.set_scoring(*SC, False, [])
    ref = _oracle("global", pairs, SC, False, [])
    for flag in ("0", "1"):
        env.setenv("AT_HOST_NO_PINNED_CALLER", flag)
        score, ei, ej, st, nops = (np.zeros(n, dtype=np.int32) for _ in range(5))
        ops = np.zeros(len(blob) + 64, dtype=np.uint8)
        P = A._ptr
        al._check(al._lib.at_align_batch(al._h, A.MODES["global"], n, C.c_void_p(pinned.data_ptr()), P(off1), P(len1), P(off2), P(len2), 1,
                                         P(score), P(ei), P(ej), P(st), P(ops), P(off1), P(nops)))
        cfg = al.last_config
        assert ("from the caller's page-locked memory" in cfg) == (flag == "0"), cfg
        for k, p in enumerate(pairs):
            r = ref[p]
            assert (int(score[k]), int(ei[k]), int(ej[k]), int(st[k])) == (r["score"], r["end_i"], r["end_j"], r["state"]), (flag, k)
            assert bytes(ops[off1[k]:off1[k] + nops[k]]) == r["ops"], (flag, k)
    env.delenv("AT_HOST_NO_PINNED_CALLER")
    # chunks side by side on helper handles
    env.delenv("AT_HOST_CHUNKS")
    env.setenv("AT_HOST_CHUNK_MIN", "64")
    uni = _batch(rng, 700, (120, 120), (140, 140))
    cfg = _run(al, "fitj", uni, ctx="chunks of 64+ pairs")
    assert cfg.endswith(" x6 chunks"), cfg
    env.setenv("AT_HOST_CHUNKS", "1")
    env.delenv("AT_HOST_CHUNK_MIN")
    # the two gapped strings rendered on the GPU with 8 .. 64 lanes per pair
    for g in ("8", "16", "32", "64"):
        env.setenv("AT_RENDER_GROUP", g)
        st = al.align_batch_strings("global", pairs[:90])
        assert "[strings: %s lanes per pair]" % g in al.last_config, al.last_config
        for k, p in enumerate(pairs[:90]):
            r = ref[p]
            assert (int(st["score"][k]), st["r1"][k], st["r2"][k]) == (r["score"], r["r1"], r["r2"]), (g, k)


# ---- C: waves that work through several items

@pytest.mark.gpu
@pytest.mark.parametrize("family", ["int32", "g8", "g16", "g32", "g64", "two-pass rounds", "walk kernel", "sliver", "ragged local",
                                    "ragged fitj", "myers"])
def test_many_items_per_wave(al, env, family):
    """The grid shrunk to a few waves (AT_WS_CAP_MB=1 with the pointers / everything in HBM, or AT_WAVES_PER_CU=1), so that every
    wave pulls at least three work items from the counter: an item's LDS, slot and registers after another item of other sequences --
    of other lengths too on the int32 kernel and in ragged frames (local: items of mixed read lengths in order of falling l2; fit:
    items of equal read length, each sweeping its own longest l2).  The uniform families (8- to 64-lane groups, two-pass, walk
    kernel, sliver) vary the sequences only.  The bit-parallel edit kernel has no such knob: a batch of more than two items per wave."""
    import zlib
    rng = random.Random(zlib.crc32(family.encode()))
    ncu = _ncu()
    tb = True
    if family == "int32":
        env.setenv("AT_NO_PACKED", "1")
        env.setenv("AT_STORE", "2")
        env.setenv("AT_WS_CAP_MB", "1")
        mode, pairs, per_wave = "fitj", _batch(rng, 150, (40, 200), (120, 300), fit=True), 1
    elif family in ("g8", "g16", "g32"):
        env.setenv("AT_TAIL_SPLIT", "0")
        env.setenv("AT_WS_CAP_MB", "1")
        l1, l2, per_wave, mode = {"g8": (150, 160, 16, "local"), "g16": (190, 200, 8, "global"), "g32": (350, 380, 4, "local")}[family]
        pairs = _batch(rng, per_wave * 40 + 3, (l1, l1), (l2, l2))
    elif family == "g64":
        env.setenv("AT_TWO_PASS", "0")
        env.setenv("AT_WS_CAP_MB", "2")
        mode, pairs, per_wave = "local", _batch(rng, 41, (640, 640), (700, 700)), 2
    elif family == "two-pass rounds":
        env.setenv("AT_TP_SPLIT", "0")
        env.setenv("AT_WS_CAP_MB", "8")
        mode, pairs, per_wave = "global", _batch(rng, 61, (1000, 1000), (1024, 1024)), 2
    elif family == "walk kernel":
        env.setenv("AT_WAVES_PER_CU", "1")
        n = 3 * 16 * ncu + 21
        uniq = _batch(rng, 331, (150, 150), (500, 500))
        mode, pairs, per_wave = "fitj", [uniq[k % len(uniq)] for k in range(n)], 16
    elif family == "ragged local":
        env.setenv("AT_WS_CAP_MB", "1")
        mode, per_wave = "local", 8            # (local frames: 16-lane groups; one rows-per-lane class, 10 rows, one bucket)
        pairs = _batch(rng, 403, (113, 160), (60, 300))
    elif family == "ragged fitj":
        env.setenv("AT_WS_CAP_MB", "1")
        mode, per_wave = "fitj", 16            # (global / fit frames: 8-lane groups; one class, 16 rows per lane)
        pairs = _batch(rng, 501, (105, 128), (105, 400), fit=True)
    elif family == "sliver":
        # main items on a grid of G waves, then one more item's worth: the last round a quarter full or less goes to 32-lane items
        env.setenv("AT_WS_CAP_MB", "1")
        mode, per_wave = "local", 16
        probe = _run(al, mode, _batch(rng, 40, (150, 150), (150, 150)), ctx="probe")
        g = (1 << 20) // int(re.search(r"slot=(\d+)B", probe).group(1))
        assert g >= 4, probe
        pairs = _batch(rng, per_wave * (3 * g + 1) - 7, (150, 150), (150, 150))
    else:
        # the 32-lane groups of the bit-parallel kernel (reads beyond AT_MYERS_LANE_MAX; AT_MYERS_LANE_MIN_PAIRS keeps a large batch off the
        # one-alignment-per-lane form): two alignments per wavefront, a batch of more than two per resident wavefront
        env.setenv("AT_MYERS_LANE_MAX", "256")
        env.setenv("AT_MYERS_LANE_MIN_PAIRS", str(1 << 30))
        mode, per_wave, tb = "edit", 2, False
        uniq = _batch(rng, 509, (257, 400), (200, 420))
        probe = _run(al, mode, uniq[:40], (1, 1, -5, -1, -10), tb=False, ctx="probe")
        occ = int(re.search(r"waves/cu<=(\d+)", probe).group(1))
        pairs = [uniq[k % len(uniq)] for k in range(2 * per_wave * occ * ncu + 5)]
    sc = (1, 1, -5, -1, -10) if mode == "edit" else SC
    if family.startswith("ragged"):
        assert len(set(pairs)) == len(pairs) and len({(len(a), len(b)) for a, b in pairs}) > len(pairs) // 2
    cfg = _run(al, mode, pairs, sc, tb=tb, sites=C4[4] if family == "walk kernel" else None, ctx=family)
    grid = _grid(cfg)
    m = re.search(r"\((\d+) pairs/wave\)", cfg)
    if m:
        assert int(m.group(1)) == per_wave, cfg
    items = -(-len(pairs) // per_wave)
    if family == "sliver":
        m = re.search(r"last (\d+) pairs as 32-lane items", cfg)
        assert m, cfg
        items = -(-(len(pairs) - int(m.group(1))) // per_wave)
    assert items >= (2 if family == "myers" else 3) * grid, (family, items, cfg)
    want = {"int32": "int32", "g8": "8x8-lane", "g16": "4x16-lane", "g32": "2x32-lane", "g64": "1x64-lane", "two-pass rounds": "two-pass ck=",
            "walk kernel": "walk kernel", "sliver": "8x8-lane", "ragged local": "4x16-lane groups (8 pairs/wave) ragged frames",
            "ragged fitj": "8x8-lane groups (16 pairs/wave) ragged frames", "myers": "2x32-lane groups"}[family]
    if family.startswith("ragged"):
        assert "(1 frames" in cfg, cfg             # (one launch: its grid is the whole batch's)
    assert want in cfg, cfg
    if family == "two-pass rounds":
        assert "walk kernel" not in cfg, cfg
