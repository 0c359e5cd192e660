"""The kernels before and after the sweep, at their edges: at_pack<2> / at_pack<8> and the host's pack2_avx2 (at_pack.hip.h,
at_hip.hip), at_render_k<BITS, W>, at_scan_tiles / at_scan_nops / at_compact_k (at_render.hip.h) and the two-part payload fetch of
the host entries.

The references are plain Python / numpy in this module and do not call the library:
  _render_ref     ops in END -> START order -> the two gapped strings in forward order
  _compact_ref    counts, slots -> exclusive int64 offsets + the payload that fits below `cap`
The CPU half (no mark) checks the references themselves -- against the host's at_render, against the reference's own strings in
tests/golden/known_answers.jsonl, against a Python loop.  The GPU half (-m gpu) drives the kernels with synthetic arrays (sections
1 and 2) or through the host entry against the oracle (sections 3 and 4).  Every comparison is exact equality, every pair of every
batch is asserted.
"""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest

import oracle as O
from conftest import load_golden

FILL = 0x7f
ACGT = b"ACGT"
BYTES = bytes(range(1, 256))


# ---------------------------------------------------------------- references

def _render_ref(ops, s1, end_i, s2, end_j):
    """ops END -> START: 0 (MID) and 1 (LOW) consume a row of s1, 0, 2 (UPP) and 3 (JUMP) a column of s2; the side that consumes
    nothing shows '-'.  Returns (r1, r2) as bytes in forward order."""
    i, j = end_i, end_j
    a, b = bytearray(), bytearray()
    for op in ops:
        if op in (0, 1):
            i -= 1
            assert i >= 0
            a.append(s1[i])
        else:
            a.append(0x2d)
        if op in (0, 2, 3):
            j -= 1
            assert j >= 0
            b.append(s2[j])
        else:
            b.append(0x2d)
    a.reverse()
    b.reverse()
    return bytes(a), bytes(b)


def _render_ref_rows(cnt, ops, s1, end_i, s2, end_j):
    """_render_ref for a whole batch at once: ops (n, S) uint8 of which the first cnt[k] count, s1 / s2 (n, L) uint8.  Returns
    (r1, r2) as (n, S) uint8, string k in row k from column 0, FILL behind it."""
    n, S = ops.shape
    valid = np.arange(S)[None, :] < cnt[:, None]
    out = []
    for seq, end, use in ((s1, end_i, valid & (ops <= 1)), (s2, end_j, valid & (ops != 1))):
        idx = end[:, None] - np.cumsum(use, axis=1)
        assert (idx[use] >= 0).all()
        ch = np.where(use, seq[np.arange(n)[:, None], np.clip(idx, 0, seq.shape[1] - 1)], 0x2d).astype(np.uint8)
        r = np.full((n, S), FILL, dtype=np.uint8)
        k, p = np.nonzero(valid)
        r[k, cnt[k] - 1 - p] = ch[k, p]
        out.append(r)
    return out[0], out[1]


def _compact_ref(nops, ops_off, ops, cap):
    """Returns (off, packed): off[n + 1] the exclusive int64 cumsum of max(nops, 0); pair k is copied to packed[off[k] ..] iff
    nops[k] > 0 and off[k] + nops[k] <= cap.  packed has min(cap, total) bytes, FILL where nothing is copied."""
    nops = np.asarray(nops, dtype=np.int64)
    ops_off = np.asarray(ops_off, dtype=np.int64)
    cnt = np.maximum(nops, 0)
    off = np.zeros(len(nops) + 1, dtype=np.int64)
    np.cumsum(cnt, out=off[1:])
    keep = (nops > 0) & (off[:-1] + nops <= cap)
    packed = np.full(int(min(cap, off[-1])), FILL, dtype=np.uint8)
    c = cnt[keep]
    if c.sum():
        within = np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c)
        packed[np.repeat(off[:-1][keep], c) + within] = ops[np.repeat(ops_off[keep], c) + within]
    return off, packed


def _synth_pair(rng, nops, alphabet):
    """(ops, s1, end_i, s2, end_j): nops random ops over {0, 1, 2, 3}, end_i <= len(s1) and end_j <= len(s2), at least as many
    rows before end_i and columns before end_j as the ops consume"""
    ops = bytes(rng.choices((0, 1, 2, 3), weights=(5, 2, 2, 1), k=nops))
    rows = sum(o <= 1 for o in ops)
    cols = sum(o != 1 for o in ops)
    end_i = rows + rng.randint(0, 3)
    end_j = cols + rng.randint(0, 3)
    s1 = bytes(rng.choices(alphabet, k=end_i + rng.randint(0, 3)))
    s2 = bytes(rng.choices(alphabet, k=end_j + rng.randint(0, 3)))
    return ops, s1, end_i, s2, end_j


def _synth_rows(seed, n, alphabet, S=12):
    """the same for a large batch, as arrays: op counts 0 .. S, sequences of S + 2 bytes"""
    rs = np.random.RandomState(seed)
    L = S + 2
    cnt = rs.randint(0, S + 1, size=n).astype(np.int32)
    ops = rs.randint(0, 4, size=(n, S)).astype(np.uint8)
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    s1 = alpha[rs.randint(0, len(alpha), size=(n, L))]
    s2 = alpha[rs.randint(0, len(alpha), size=(n, L))]
    valid = np.arange(S)[None, :] < cnt[:, None]
    end_i = ((valid & (ops <= 1)).sum(axis=1) + rs.randint(0, 3, size=n)).astype(np.int32)
    end_j = ((valid & (ops != 1)).sum(axis=1) + rs.randint(0, 3, size=n)).astype(np.int32)
    return cnt, ops, s1, end_i, s2, end_j


# ---------------------------------------------------------------- 0. CPU half

def test_render_ref_equals_host_render():
    import aligntools.c_amd as A
    lib = A.load_library()
    rng = random.Random(5)
    ncases = 0
    for alphabet in (ACGT, BYTES):
        for _ in range(2000):
            ops, s1, end_i, s2, end_j = _synth_pair(rng, rng.choice((0, 1, 2, 15, 16, 17, 64, rng.randint(0, 200))), alphabet)
            n = len(ops)
            r1, r2 = C.create_string_buffer(n + 1), C.create_string_buffer(n + 1)
            assert lib.at_render(ops, n, s1, end_i, s2, end_j, r1, r2) == 0
            assert (r1.raw[:n], r2.raw[:n]) == _render_ref(ops, s1, end_i, s2, end_j), (ops, s1, end_i, s2, end_j)
            assert r1.raw[n] == 0 and r2.raw[n] == 0
            ncases += 1
    assert ncases == 4000


def test_render_ref_reproduces_the_reference_strings():
    """r1 / r2 of every golden case (made by the reference itself) from the oracle's ops and end cell"""
    ncases = 0
    for c in load_golden("known_answers.jsonl"):
        if c["mode"] == "edit":
            continue
        r = O.align(O.MODE_NAMES[c["mode"]], c["s1"], c["s2"], c["m"], c["u"], c["o"], c["e"], c["j"], c["use_jump"], c["sites"])
        assert r["rc"] == 0 and r["score"] == c["score"], c["tag"]
        got = _render_ref(r["ops"], c["s1"].encode("latin1"), r["end_i"], c["s2"].encode("latin1"), r["end_j"])
        if "r1" in c:
            assert got == (c["r1"].encode("latin1"), c["r2"].encode("latin1")), (c["tag"], c["mode"])
        else:                                          # (long strings are kept as their length and digests)
            assert len(got[0]) == len(got[1]) == c["rlen"], (c["tag"], c["mode"])
            assert (hashlib.md5(got[0]).hexdigest(), hashlib.md5(got[1]).hexdigest()) == (c["r1_md5"], c["r2_md5"]), (c["tag"], c["mode"])
        ncases += 1
    assert ncases >= 25


def test_render_ref_rows_equals_render_ref():
    for alphabet in (ACGT, BYTES):
        cnt, ops, s1, end_i, s2, end_j = _synth_rows(9, 3000, alphabet)
        r1, r2 = _render_ref_rows(cnt, ops, s1, end_i, s2, end_j)
        assert set(cnt.tolist()) == set(range(13))
        for k in range(len(cnt)):
            n = int(cnt[k])
            want = _render_ref(ops[k, :n].tobytes(), s1[k].tobytes(), int(end_i[k]), s2[k].tobytes(), int(end_j[k]))
            assert (r1[k, :n].tobytes(), r2[k, :n].tobytes()) == want, k
            assert (r1[k, n:] == FILL).all() and (r2[k, n:] == FILL).all()


def test_compact_ref_equals_a_loop():
    rng = random.Random(6)
    for n in (0, 1, 2, 3, 7, 50):
        for _ in range(40):
            nops = np.array([rng.choice((-5, -1, 0, 0, 1, 2, 3, 6)) for _ in range(n)], dtype=np.int32)
            ops_off = np.array(rng.sample(range(n), n), dtype=np.int64) * 6
            ops = np.array([rng.randrange(256) for _ in range(6 * n)], dtype=np.uint8)
            total = int(np.maximum(nops, 0).sum())
            for cap in (total + 10, total, total // 2, 1, 0):
                off, packed = _compact_ref(nops, ops_off, ops, cap)
                want_off, run = [], 0
                want = [FILL] * min(cap, total)
                for k in range(n):
                    want_off.append(run)
                    c = max(int(nops[k]), 0)
                    if c > 0 and run + c <= cap:
                        want[run:run + c] = ops[ops_off[k]:ops_off[k] + c].tolist()
                    run += c
                want_off.append(run)
                assert off.dtype == np.int64 and off.tolist() == want_off
                assert packed.tolist() == want, (n, cap)


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


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- 1. rendering kernel, synthetic ops

def _slots(rng, sizes):
    """byte offsets of slots of the given sizes laid out back to back in a random order of the pairs; returns (offsets, total)"""
    order = list(range(len(sizes)))
    rng.shuffle(order)
    off = [0] * len(sizes)
    at = 0
    for k in order:
        off[k] = at
        at += sizes[k]
    return np.array(off, dtype=np.int64), at


class _RenderBatch:
    """Synthetic pairs with the given op counts.  Every 11th pair (k % 11 == 5) is flagged: nops = -1, and its ops_off, str_off,
    woff and end entries are those of the pair before it (in bounds, and somebody else's); its own slots must keep their fill."""

    def __init__(self, seed, counts, bits):
        import aligntools.c_amd as A
        rng = random.Random(seed)
        n = len(counts)
        self.n = n
        self.cases = [_synth_pair(rng, c, ACGT if bits == 2 else BYTES) for c in counts]
        self.want = [_render_ref(*c) for c in self.cases]
        self.flagged = [n > 1 and k % 11 == 5 for k in range(n)]
        words, woff1, woff2, _len1, _len2, got = A.pack_pairs([(c[1], c[3]) for c in self.cases], bits=bits)
        assert got == bits
        nops = np.array(counts, dtype=np.int32)
        end_i = np.array([c[2] for c in self.cases], dtype=np.int32)
        end_j = np.array([c[4] for c in self.cases], dtype=np.int32)
        self.str_off, str_total = _slots(rng, [c + 1 + rng.randint(0, 5) for c in counts])
        self.ops_off, ops_total = _slots(rng, [c + 1 + rng.randint(0, 3) for c in counts])
        ops = np.full(ops_total + 64, 0xee, dtype=np.uint8)          # (0xee between the lists: not an op)
        for k, c in enumerate(self.cases):
            ops[self.ops_off[k]:self.ops_off[k] + counts[k]] = np.frombuffer(c[0], dtype=np.uint8)
        self.size = max(str_total, ops_total) + 64
        arg = {"nops": nops, "end_i": end_i, "end_j": end_j, "woff1": woff1, "woff2": woff2,
               "str_off": self.str_off.copy(), "ops_off": self.ops_off.copy()}
        for k in range(n):
            if self.flagged[k]:
                for name, a in arg.items():
                    a[k] = -1 if name == "nops" else a[k - 1]
        self.d = {name: _dev(a) for name, a in arg.items()}
        self.d["words"] = _dev(words.view(np.int32))
        self.d["ops"] = _dev(ops)
        self.bits = bits

    def expected(self, off, nul):
        w1 = np.full(self.size, FILL, dtype=np.uint8)
        w2 = np.full(self.size, FILL, dtype=np.uint8)
        for k, (a, b) in enumerate(self.want):
            if self.flagged[k]:
                continue
            o, n = int(off[k]), len(a)
            w1[o:o + n] = np.frombuffer(a, dtype=np.uint8)
            w2[o:o + n] = np.frombuffer(b, dtype=np.uint8)
            if nul:
                w1[o + n] = 0
                w2[o + n] = 0
        return w1, w2

    def run(self, al, use_str_off, nul):
        import torch
        d = self.d
        d_r1 = torch.full((self.size,), FILL, dtype=torch.uint8, device=d["ops"].device)
        d_r2 = torch.full((self.size,), FILL, dtype=torch.uint8, device=d["ops"].device)
        al.render_batch_device(self.n, d["words"].data_ptr(), self.bits, d["woff1"].data_ptr(), d["woff2"].data_ptr(),
                               d["end_i"].data_ptr(), d["end_j"].data_ptr(), d["ops"].data_ptr(), d["ops_off"].data_ptr(),
                               d["nops"].data_ptr(), d_r1.data_ptr(), d_r2.data_ptr(),
                               d["str_off"].data_ptr() if use_str_off else None, nul, _stream())
        torch.cuda.synchronize()
        return d_r1.cpu().numpy(), d_r2.cpu().numpy()

    def check(self, al, ctx):
        """all four of (str_off given / NULL) x (terminated / not): the strings, the byte behind each, every other byte of both
        buffers.  Returns the number of strings compared."""
        for use_str_off in (True, False):
            off = self.str_off if use_str_off else self.ops_off
            for nul in (True, False):
                g1, g2 = self.run(al, use_str_off, nul)
                w1, w2 = self.expected(off, nul)
                if not (np.array_equal(g1, w1) and np.array_equal(g2, w2)):
                    for k, (a, b) in enumerate(self.want):       # (which pair: for the message)
                        o, n = int(off[k]), len(a) + 1
                        assert (g1[o:o + n].tobytes(), g2[o:o + n].tobytes()) == (w1[o:o + n].tobytes(), w2[o:o + n].tobytes()), \
                            (ctx, "str_off" if use_str_off else "NULL", nul, "pair", k, "nops", n - 1, "flagged", self.flagged[k])
                    bad = np.nonzero((g1 != w1) | (g2 != w2))[0]
                    raise AssertionError((ctx, use_str_off, nul, "bytes outside every string changed", bad[:8].tolist()))
        return 4 * 2 * (self.n - sum(self.flagged))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [8, 16, 32, 64])
@pytest.mark.parametrize("bits", [2, 8])
def test_render_kernel_edge_batch(al, monkeypatch, bits, W):
    """Op counts on both sides of every multiple of the group width, short and long lists side by side in every wavefront, flagged
    pairs inside groups, an odd number of pairs, slots at odd offsets in a random order, and one-pair batches."""
    monkeypatch.setenv("AT_RENDER_GROUP", str(W))
    rng = random.Random(1000 * bits + W)
    npairs = 2001
    special = [0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 63, 64, 65, 127, 128, 129, 200]
    counts = (special * (npairs // 2 // len(special) + 1))[:npairs // 2]
    counts += [rng.randint(0, 200) for _ in range(npairs - len(counts))]
    rng.shuffle(counts)
    assert len(counts) % 2 == 1 and set(special) <= set(counts)
    b = _RenderBatch(rng.random(), counts, bits)
    assert sum(b.flagged) == 182
    nstr = b.check(al, ("edge batch", bits, W))
    for c in (0, 1, 2 * W + 1, 200):
        nstr += _RenderBatch(rng.random(), [c], bits).check(al, ("one pair", bits, W, c))
    print("render edge batch bits=%d W=%d: %d strings compared" % (bits, W, nstr))


_grid_cache = {}


def _grid_batch(bits, nmax):
    """The grid-stride batch at its largest size (W = 8), made and packed once per word size; a narrower launch takes a prefix."""
    import aligntools.c_amd as A
    if bits not in _grid_cache:
        cnt, ops, s1, end_i, s2, end_j = _synth_rows(40 + bits, nmax, ACGT if bits == 2 else BYTES)
        r1, r2 = _render_ref_rows(cnt, ops, s1, end_i, s2, end_j)
        words, woff1, woff2, _l1, _l2, got = A.pack_pairs([(s1[k].tobytes(), s2[k].tobytes()) for k in range(nmax)], bits=bits)
        assert got == bits
        d = {"words": _dev(words.view(np.int32)), "woff1": _dev(woff1), "woff2": _dev(woff2), "end_i": _dev(end_i), "end_j": _dev(end_j),
             "nops": _dev(cnt), "ops": _dev(ops.reshape(-1)), "ops_off": _dev(np.arange(nmax, dtype=np.int64) * ops.shape[1])}
        _grid_cache[bits] = (d, r1, r2)
    return _grid_cache[bits]


@pytest.mark.gpu
@pytest.mark.parametrize("W", [8, 16, 32, 64])
@pytest.mark.parametrize("bits", [2, 8])
def test_render_kernel_grid_stride(al, monkeypatch, bits, W):
    """37 pairs more than one pass of the full grid: the second trip of every wavefront's loop over the pairs."""
    import torch
    monkeypatch.setenv("AT_RENDER_GROUP", str(W))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 16 * ncu * 4 * (64 // W) + 37
    d, r1, r2 = _grid_batch(bits, 16 * ncu * 4 * 8 + 37)
    S = r1.shape[1]
    d_r1 = torch.full((n * S + 64,), FILL, dtype=torch.uint8, device=d["ops"].device)
    d_r2 = torch.full((n * S + 64,), FILL, dtype=torch.uint8, device=d["ops"].device)
    al.render_batch_device(n, d["words"].data_ptr(), bits, d["woff1"].data_ptr(), d["woff2"].data_ptr(), d["end_i"].data_ptr(),
                           d["end_j"].data_ptr(), d["ops"].data_ptr(), d["ops_off"].data_ptr(), d["nops"].data_ptr(),
                           d_r1.data_ptr(), d_r2.data_ptr(), None, False, _stream())
    torch.cuda.synchronize()
    g1, g2 = d_r1.cpu().numpy(), d_r2.cpu().numpy()
    for g, r in ((g1, r1), (g2, r2)):
        diff = np.nonzero((g[:n * S].reshape(n, S) != r[:n]).any(axis=1))[0]
        assert len(diff) == 0, (bits, W, "pairs", diff[:8].tolist(), "of", n)
        assert (g[n * S:] == FILL).all()
    print("render grid-stride bits=%d W=%d: %d strings compared" % (bits, W, 2 * n))


# ---- 2. scan and compaction, synthetic counts

def _compact_run(al, n, d_nops, d_ops_off, d_ops, size, cap):
    import torch
    d_packed = torch.full((size,), FILL, dtype=torch.uint8, device=d_ops.device)
    d_off = torch.full((n + 3,), -77, dtype=torch.int64, device=d_ops.device)
    al.compact_ops_device(n, d_ops.data_ptr(), d_ops_off.data_ptr(), d_nops.data_ptr(), d_packed.data_ptr(), cap, d_off.data_ptr(),
                          _stream())
    torch.cuda.synchronize()
    off = d_off.cpu().numpy()
    assert (off[n + 1:] == -77).all(), (n, cap, "offsets written behind off[n]")
    return off[:n + 1], d_packed.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 255, 256, 257, 1023, 1024, 1025, 4097, 600001])
def test_scan_and_compaction(al, n):
    """Counts in 0 .. 6 with some -1 and -5, slots of 6 bytes in a shuffled order: offsets and payload with room to spare, and the
    `cap` rule at half the total and at 0."""
    rs = np.random.RandomState(n)
    nops = rs.randint(0, 7, size=n).astype(np.int32)
    x = rs.randint(0, 20, size=n)
    nops[x == 0] = -1
    nops[x == 1] = -5
    if n >= 63:
        assert (nops == -1).any() and (nops == -5).any() and (nops == 6).any()
    ops_off = rs.permutation(n).astype(np.int64) * 6
    ops = rs.randint(0, 256, size=6 * n).astype(np.uint8)
    total = int(np.maximum(nops, 0).sum())
    d_nops, d_ops_off, d_ops = _dev(nops), _dev(ops_off), _dev(ops)
    size = total + 64
    ncopied = 0
    for cap in (size, total // 2, 0):
        want_off, want = _compact_ref(nops, ops_off, ops, cap)
        assert want_off[-1] == total
        off, packed = _compact_run(al, n, d_nops, d_ops_off, d_ops, size, cap)
        assert np.array_equal(off, want_off), (n, cap, np.nonzero(off != want_off)[0][:8].tolist())
        assert np.array_equal(packed[:len(want)], want), (n, cap, np.nonzero(packed[:len(want)] != want)[0][:8].tolist())
        assert (packed[len(want):] == FILL).all(), (n, cap, "bytes at or behind cap written")
        if cap == size:
            assert len(want) == total and (n < 63 or not (want == FILL).all())
        ncopied += int(((nops > 0) & (want_off[:-1] + nops <= cap)).sum())
    print("scan/compaction n=%d: 3 x %d offsets, %d pairs copied, total %d" % (n, n + 1, ncopied, total))


@pytest.mark.gpu
def test_scan_totals_beyond_32_bits(al):
    """4 096 counts of 2^30: offsets up to 2^42, and with cap = 0 nothing is copied"""
    import torch
    n = 4096
    nops = np.full(n, 1 << 30, dtype=np.int32)
    d_ops = torch.full((64,), 3, dtype=torch.uint8, device=torch.device("cuda", 0))
    off, packed = _compact_run(al, n, _dev(nops), _dev(np.zeros(n, dtype=np.int64)), d_ops, 64, 0)
    want = np.arange(n + 1, dtype=np.int64) << 30
    assert want[-1] == 1 << 42
    assert np.array_equal(off, want), np.nonzero(off != want)[0][:8].tolist()
    assert (packed == FILL).all()


@pytest.mark.gpu
def test_compaction_of_no_pairs(al):
    import torch
    dev = torch.device("cuda", 0)
    d_packed = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    d_off = torch.full((4,), -77, dtype=torch.int64, device=dev)
    d_nops = torch.full((4,), 5, dtype=torch.int32, device=dev)
    d_ops_off = torch.zeros(4, dtype=torch.int64, device=dev)
    d_ops = torch.zeros(64, dtype=torch.uint8, device=dev)
    al.compact_ops_device(0, d_ops.data_ptr(), d_ops_off.data_ptr(), d_nops.data_ptr(), d_packed.data_ptr(), 64, d_off.data_ptr(),
                          _stream())
    torch.cuda.synchronize()
    assert d_off.cpu().tolist() == [0, -77, -77, -77]
    assert (d_packed.cpu().numpy() == FILL).all()


# ---- 3. alphabet detection and packing through the host entry

SC = (2, -2, -5, -2)          # mild: every base matters, and the scores stay far from what forces byte words
ROUTES = ["default", "device pack", "page-locked"]
_ref_cache = {}


def _ref(p):
    if p not in _ref_cache:
        r = O.align(O.GLOBAL, p[0], p[1], *SC)
        assert r["rc"] == 0
        _ref_cache[p] = r
    return _ref_cache[p]


class _HostEntry:
    """at_align_batch (global, SC) by one of the three upload routes: "default" (the host's 2-bit packing first), "device pack"
    (AT_HOST_PACK=0: raw bytes up, at_pack<2> finds the alphabet) or "page-locked" (the caller's blob in page-locked memory)."""

    def __init__(self, al, monkeypatch, route):
        import torch
        self.al, self.route = al, route
        monkeypatch.setenv("AT_HOST_CHUNKS", "1")     # (a chunk on a helper handle would keep its own last_config)
        if route == "device pack":
            monkeypatch.setenv("AT_HOST_PACK", "0")
        self.pinned = torch.empty(1 << 16, dtype=torch.uint8).pin_memory() if route == "page-locked" else None
        al.set_scoring(*SC)

    def __call__(self, pairs):
        """Returns (result dict with score, end_i, end_j, state, ops, last_config)."""
        import torch
        import aligntools.c_amd as A
        al = self.al
        if self.route != "page-locked":
            res = al.align_batch("global", pairs, render=False)
            return res, al.last_config
        blob, off1, len1, off2, len2 = A._flatten(pairs)
        n = len(pairs)
        assert len(blob) <= len(self.pinned)
        self.pinned[:len(blob)].copy_(torch.from_numpy(blob))
        score, ei, ej, st, nops = (np.zeros(n, dtype=np.int32) for _ in range(5))
        ops = np.zeros(len(blob) + 64, dtype=np.uint8)
        P = A._ptr
        al._check(al._lib.at_align_batch(al._h, A.MODES["global"], n, C.c_void_p(self.pinned.data_ptr()), P(off1), P(len1), P(off2),
                                         P(len2), 1, P(score), P(ei), P(ej), P(st), P(ops), P(off1), P(nops)))
        cfg = al.last_config
        assert "from the caller's page-locked memory" in cfg, cfg
        return dict(score=score, end_i=ei, end_j=ej, state=st, ops=[bytes(ops[off1[k]:off1[k] + nops[k]]) for k in range(n)]), cfg


def _assert_pairs(res, pairs, ctx):
    for k, p in enumerate(pairs):
        r = _ref(p)
        assert (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), int(res["state"][k])) == \
            (r["score"], r["end_i"], r["end_j"], r["state"]), (ctx, "pair", k, p)
        assert res["ops"][k] == r["ops"], (ctx, "pair", k, p)
    return len(pairs)


def _pure(rng, n):
    return bytes(rng.choices(ACGT, k=n))


def _foreign_call(run, rng, L, p, b, align, victim_is_s2):
    """One call: `align` filler pairs of 5 bases each, then the four pairs (v, v with v[p] := X), X in ACGT, where v is pure ACGT
    but for byte b at p.  A byte packed as base X makes pair X a perfect match; the oracle sees a mismatch in all four.  Returns
    (pairs asserted, the blob offsets of the four victims, whether the foreign byte is the last byte of the blob)."""
    pairs = [(_pure(rng, 2), _pure(rng, 3)) for _ in range(align)]
    v = bytearray(_pure(rng, L))
    v[p] = b
    v = bytes(v)
    at, offs = 5 * align, []
    for x in ACGT:
        w = bytearray(v)
        w[p] = x
        pairs.append((bytes(w), v) if victim_is_s2 else (v, bytes(w)))
        offs.append(at + (L if victim_is_s2 else 0))
        at += 2 * L
    res, cfg = run(pairs)
    ctx = (run.route, "L", L, "p", p, "byte", b, "victim offsets", offs, "victim is s2" if victim_is_s2 else "victim is s1", cfg)
    assert "bits=8" in cfg, ctx
    for k in range(align, align + 4):                 # (said before the oracle comparison: what a miscoded byte looks like)
        assert int(res["score"][k]) != 2 * L, ("a foreign byte was taken for a base",) + ctx
    return _assert_pairs(res, pairs, ctx), offs, victim_is_s2 and p == L - 1


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_one_foreign_byte_at_every_position(al, monkeypatch, route):
    """'N' at every dword, word and 32-byte-step boundary, in the tail and as the last byte of the blob, the sequence at each of
    the four byte alignments, as s1 and as s2: the batch goes to byte words and every pair equals the oracle."""
    run = _HostEntry(al, monkeypatch, route)
    rng = random.Random(31)
    npairs = ncalls = 0
    last_of_blob = False
    for L in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 70):
        for p in sorted({q for q in (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, L - 2, L - 1) if 0 <= q < L}):
            for victim_is_s2 in (False, True):
                seen = set()
                for align in range(4):
                    n, offs, last = _foreign_call(run, rng, L, p, ord("N"), align, victim_is_s2)
                    seen.add(offs[0] % 4)
                    npairs += n
                    ncalls += 1
                    last_of_blob |= last
                assert seen == {0, 1, 2, 3}, (L, p, seen)
    assert last_of_blob
    print("foreign byte, positions, %s: %d calls, %d pairs asserted" % (route, ncalls, npairs))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_one_foreign_byte_of_every_value(al, monkeypatch, route):
    """Every byte 1 .. 255 but ACGT (0 ends a C string: the oracle cannot take it) at base 37 of 45 -- in the tail of the host's
    32-byte steps, second byte of its dword -- among them the bytes whose code bits are a base's ('a', 'c', 'g', 't', 'E', ...)."""
    run = _HostEntry(al, monkeypatch, route)
    rng = random.Random(32)
    npairs = ncalls = 0
    for b in range(1, 256):
        if b in ACGT:
            continue
        for victim_is_s2 in (False, True):
            n, _offs, _last = _foreign_call(run, rng, 45, 37, b, (b + victim_is_s2) % 4, victim_is_s2)
            npairs += n
            ncalls += 1
    assert ncalls == 2 * 251
    print("foreign byte, values, %s: %d calls, %d pairs asserted" % (route, ncalls, npairs))


def _mutated(rng, a, length):
    """a with a few substitutions, then bases inserted or deleted until it has `length` bases"""
    t = bytearray(a)
    for _ in range(1 + len(t) // 12):
        t[rng.randrange(len(t))] = rng.choice(ACGT)
    while len(t) < length:
        t.insert(rng.randrange(len(t) + 1), rng.choice(ACGT))
    while len(t) > length:
        del t[rng.randrange(len(t))]
    return bytes(t)


@pytest.mark.gpu
@pytest.mark.parametrize("pack", ["default", "device pack"])
def test_foreign_byte_in_a_late_chunk(al, monkeypatch, pack):
    """700 uniform pairs in chunks of 64 and more on helper handles; the batch's only foreign byte is in the last pair, so the
    chunks before it keep their 2-bit words and the last one changes to byte words on its own."""
    monkeypatch.delenv("AT_HOST_CHUNKS", raising=False)
    monkeypatch.setenv("AT_HOST_CHUNK_MIN", "64")
    if pack == "device pack":
        monkeypatch.setenv("AT_HOST_PACK", "0")
    rng = random.Random(33)
    pairs = []
    for _ in range(700):
        a = _pure(rng, 120)
        pairs.append((a, _mutated(rng, a + _pure(rng, 20), 140)))
    a, b = pairs[-1]
    pairs[-1] = (a, b[:77] + b"N" + b[78:])
    al.set_scoring(*SC)
    res = al.align_batch("global", pairs, render=False)
    cfg = al.last_config
    assert cfg.endswith(" x6 chunks"), cfg
    n = _assert_pairs(res, pairs, (pack, cfg))
    print("foreign byte in a late chunk, %s: %d pairs asserted" % (pack, n))


def _every_length_and_alignment(seed):
    """Pairs (a, mutated a) with len(a) running over 1 .. 80 four times, the length of the mutated copy chosen so that the next a
    starts at a byte alignment its length has not had yet.  (A length that occurs twice cannot have had four alignments: four
    rounds are the fewest.)  Returns the pairs; asserts that every length has been at all four alignments."""
    rng = random.Random(seed)
    pairs, at = [], 0
    seen = {L: set() for L in range(1, 81)}
    lengths = list(range(1, 81)) * 4
    for q, L in enumerate(lengths):
        assert at % 4 not in seen[L]
        seen[L].add(at % 4)
        a = _pure(rng, L)
        nxt = lengths[q + 1] if q + 1 < len(lengths) else None
        for L2 in ((L, L + 1, L + 2, L + 3) if L < 2 else (L - 1, L, L + 1, L + 2)):
            if nxt is None or (at + L + L2) % 4 == min(set(range(4)) - seen[nxt]):
                break
        pairs.append((a, _mutated(rng, a, L2)))
        at += L + L2
    assert all(s == {0, 1, 2, 3} for s in seen.values())
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pure, default", "pure, device pack", "N at the end, default", "N at the end, device pack"])
def test_clean_pack_of_every_length_and_alignment(al, monkeypatch, case):
    """Sequences of 1 .. 80 bases at each of the four byte alignments in the blob: packed by the host's pack2_avx2 (its tail of 1 .. 31
    bases), by at_pack<2>, and -- with one N as the very last base of the batch -- by at_pack<8> (its `left < 4` mask on every
    sequence before it)."""
    monkeypatch.setenv("AT_HOST_CHUNKS", "1")
    if "device pack" in case:
        monkeypatch.setenv("AT_HOST_PACK", "0")
    pairs = _every_length_and_alignment(34)
    assert len(pairs) == 320
    if case.startswith("N"):
        a, b = pairs[-1]
        pairs[-1] = (a, b + b"N")
    al.set_scoring(*SC)
    res = al.align_batch("global", pairs, render=False)
    cfg = al.last_config
    if case == "pure, default":
        assert "packed on the host" in cfg, cfg
    else:
        assert "raw bytes staged" in cfg, cfg
    assert ("bits=8" in cfg) == case.startswith("N"), cfg
    n = _assert_pairs(res, pairs, (case, cfg))
    print("every length and alignment, %s: %d pairs asserted" % (case, n))


# ---- 4. strings entry: payload fetched in two parts

@pytest.mark.gpu
def test_payload_fetched_in_two_parts():
    """A handle whose last batch was tiny fetches 64 kB of payload with the results and the rest behind a second wait: 700 global
    pairs of 200 x 210 (about 150 kB of strings, and of ops) after 3 short local pairs, through both entries, and the small batch
    again after each.  The small batch has a local pair of score 0 -- for which the reference still walks one cell back: strings of
    one character -- and is followed by three overlap pairs whose alignments are empty."""
    import aligntools.c_amd as A
    rng = random.Random(41)
    small = [("AAAA", "CCCC"), ("PLEASANTLY", "MEANLY"), ("ACGTACGTTGCA", "TTACGTACGAAGCA")]
    empty = [("PLEASANTLY", "MEANLY"), ("AAAA", "CCCC"), ("ACGTT", "GGACG")]
    big = []
    for _ in range(700):
        a = _pure(rng, 200)
        big.append((a.decode(), _mutated(rng, a, 210).decode()))
    want_small = [O.align(O.LOCAL, a, b, *SC) for a, b in small]
    want_empty = [O.align(O.OVERLAP, a, b, *SC) for a, b in empty]
    want_big = [O.align(O.GLOBAL, a, b, *SC) for a, b in big]
    assert want_small[0]["score"] == 0 and len(want_small[0]["ops"]) == 1
    assert all(r["rc"] == 0 and (r["r1"], r["r2"], r["ops"]) == ("", "", b"") for r in want_empty)
    assert sum(len(r["ops"]) for r in want_big) > 140000

    def check(res, want, strings, ctx):
        for k, r in enumerate(want):
            assert r["rc"] == 0
            assert (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k])) == (r["score"], r["end_i"], r["end_j"]), (ctx, k)
            if strings:
                assert (res["r1"][k], res["r2"][k]) == (r["r1"], r["r2"]), (ctx, k)
            else:
                assert res["ops"][k] == r["ops"], (ctx, k)
        return len(want)

    h = A.Aligner()
    n = 0
    try:
        h.set_scoring(*SC)
        for strings in (True, False):
            entry = (lambda mode, pairs: h.align_batch_strings(mode, pairs)) if strings else \
                    (lambda mode, pairs: h.align_batch(mode, pairs, render=False))
            n += check(entry("local", small), want_small, strings, ("small, before", strings))
            n += check(entry("global", big), want_big, strings, ("big", strings))
            n += check(entry("local", small), want_small, strings, ("small, after", strings))
            n += check(entry("overlap", empty), want_empty, strings, ("empty alignments", strings))
    finally:
        h.close()
    assert n == 2 * (700 + 9)
    print("payload in two parts: %d pairs asserted" % n)
