"""Run-length CIGARs and alignment statistics: the host helper at_cigar, the kernel behind at_cigar_batch_device and the host entry
at_align_batch_cigar (include/aligntools_hip.h, csrc/at_cigar.hip).

The rule is restated here in a dozen lines of Python (_cigar_ref).  The CPU half holds at_cigar to it and, through the oracle's op
lists, to the real reference's own gapped strings in tests/golden.  The GPU half (-m gpu) drives the kernel with crafted op lists
on both sides of every pass boundary and expects what at_cigar gives; every comparison is exact equality."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import oracle as O
from conftest import load_golden

import aligntools.c_amd as A

FILL = 0x7f7f7f7f
EQ, NE, INS, DEL, SKIP = 7, 8, 1, 2, 3


# ---------------------------------------------------------------- the rule, restated

def _cigar_ref(ops, s1, end_i, s2, end_j, extended=True):
    """ops END -> START.  Returns (words in reading order, the eight statistics), or None for an inconsistent list."""
    i, j, runs, st = end_i, end_j, [], [0] * 8
    for op in ops:
        if op > 3:
            return None
        i -= op <= 1
        j -= op != 1
        if i < 0 or j < 0:
            return None
        cls = (EQ if s1[i] == s2[j] else NE) if op == 0 else op
        st[{EQ: 2, NE: 3, INS: 4, DEL: 5, SKIP: 6}[cls]] += 1
        rc = 0 if cls >= EQ and not extended else cls
        if runs and runs[-1][0] == rc:
            runs[-1][1] += 1
        else:
            runs.append([rc, 1])
            st[7] += cls in (INS, DEL)
    st[0], st[1] = i, j
    return [(n << 4) | c for c, n in reversed(runs)], st


def _host(ops, s1, end_i, s2, end_j, extended=True, want_words=True):
    """at_cigar through ctypes: (rc, ncigar, words, stats)"""
    lib = A.load_library()
    words = (C.c_uint32 * max(1, len(ops)))(*([FILL] * max(1, len(ops))))
    stats = (C.c_int32 * 8)()
    nc = C.c_int32(12345)
    rc = lib.at_cigar(bytes(ops), len(ops), bytes(s1), end_i, bytes(s2), end_j, 0 if extended else A.CIGAR_M,
                      words if want_words else None, C.byref(nc), stats)
    return rc, nc.value, list(words), list(stats)


def _synth_pair(rng, nops, alphabet, weights=(5, 2, 2, 1)):
    ops = bytes(rng.choices((0, 1, 2, 3), weights=weights, k=nops))
    rows = sum(o <= 1 for o in ops)
    cols = sum(o != 1 for o in ops)
    end_i = rows + rng.randint(0, 3)
    end_j = cols + rng.randint(0, 3)
    s1 = bytes(rng.choices(alphabet, k=end_i + rng.randint(0, 3)))
    s2 = bytes(rng.choices(alphabet, k=end_j + rng.randint(0, 3)))
    return ops, s1, end_i, s2, end_j


# ---------------------------------------------------------------- CPU half

def test_host_cigar_equals_the_restatement():
    rng = random.Random(17)
    cases = [_synth_pair(rng, rng.choice((0, 1, 2, 15, 16, 17, 64, rng.randint(0, 200))), alpha, w)
             for alpha in (b"ACGT", b"AC", bytes(range(1, 256))) for w in ((5, 2, 2, 1), (30, 1, 1, 1)) for _ in range(500)]
    cases.append((b"", b"ACG", 2, b"ACGT", 3))                                   # the empty list: start = end
    cases += [(bytes([op]), b"AC", 2, b"AG", 2) for op in (0, 1, 2, 3)]          # a single op
    cases.append((bytes(5000), b"A" * 5000, 5000, b"A" * 5001, 5001))            # one run of 5 000 equal columns
    for ops, s1, end_i, s2, end_j in cases:
        for extended in (True, False):
            want_words, want_stats = _cigar_ref(ops, s1, end_i, s2, end_j, extended)
            rc, nc, words, stats = _host(ops, s1, end_i, s2, end_j, extended)
            assert rc == 0 and nc == len(want_words), (ops, s1, end_i, s2, end_j)
            assert words[:nc] == want_words and stats == want_stats, (ops, s1, end_i, s2, end_j, extended)
            assert all(w == FILL for w in words[max(nc, 1):])
            # counts and statistics alone, without a buffer for the words
            rc, nc2, _w, stats2 = _host(ops, s1, end_i, s2, end_j, extended, want_words=False)
            assert (rc, nc2, stats2) == (0, nc, want_stats)
    w, st = _cigar_ref(bytes(5000), b"A" * 5000, 5000, b"A" * 5001, 5001)
    assert w == [(5000 << 4) | EQ] and st == [0, 1, 5000, 0, 0, 0, 0, 0]
    assert _cigar_ref(b"", b"ACG", 2, b"ACGT", 3) == ([], [2, 3, 0, 0, 0, 0, 0, 0])
    # the module-level wrappers
    words, stats = A.cigar(bytes([0, 0, 1, 0, 2, 2, 0]), b"ACGTA", 5, b"ACCGTA", 6)
    assert A.cigar_string(words) == b"1=2D1X1I2=" and stats.tolist() == [0, 0, 3, 1, 1, 2, 0, 2]
    words, _ = A.cigar(bytes([0, 0, 1, 0, 2, 2, 0]), b"ACGTA", 5, b"ACCGTA", 6, extended=False)
    assert A.cigar_string(words) == b"1M2D1M1I2M"
    assert A.cigar_string([(12 << 4) | 7, (1 << 4) | 8, (3 << 4) | 1, (40 << 4) | 7]) == b"12=1X3I40="


def _expand(words, s1, start_i, s2, start_j):
    """CIGAR words over the two sequences -> the two gapped strings (I: '-' in the second, D / N: '-' in the first)"""
    i, j, a, b = start_i, start_j, [], []
    for w in words:
        n, c = w >> 4, w & 15
        assert n > 0 and c in (EQ, NE, INS, DEL, SKIP)
        a.append(s1[i:i + n] if c in (EQ, NE, INS) else "-" * n)
        b.append(s2[j:j + n] if c != INS else "-" * n)
        if c in (EQ, NE):
            assert all((x == y) == (c == EQ) for x, y in zip(s1[i:i + n], s2[j:j + n]))
        i += n if c in (EQ, NE, INS) else 0
        j += n if c != INS else 0
    return "".join(a), "".join(b), i, j


def test_cigars_of_the_goldens_expand_to_the_reference_strings():
    ncases = nskip_runs = 0
    for name in ("known_answers.jsonl", "random_small.jsonl", "random_dna.jsonl", "dense_sites.jsonl"):
        for c in load_golden(name):
            if c["mode"] == "edit":
                continue
            r = O.align(O.MODE_NAMES[c["mode"]], c["s1"], c["s2"], c["m"], c["u"], c["o"], c["e"], c["j"], c["use_jump"], c["sites"])
            assert r["rc"] == 0 and r["score"] == c["score"], c["tag"]
            assert (O.OP_MID, O.OP_LOW, O.OP_UPP, O.OP_JUMP) == (A.OP_MID, A.OP_LOW, A.OP_UPP, A.OP_JUMP)
            s1, s2 = c["s1"].encode("latin1"), c["s2"].encode("latin1")
            rc, nc, words, st = _host(bytes(r["ops"]), s1, r["end_i"], s2, r["end_j"])
            assert rc == 0, c["tag"]
            words = words[:nc]
            r1, r2, ei, ej = _expand(words, c["s1"], st[0], c["s2"], st[1])
            assert (ei, ej) == (r["end_i"], r["end_j"]), c["tag"]
            if "r1" in c:
                assert (r1, r2) == (c["r1"], c["r2"]), (name, c["tag"], c["mode"])
            else:
                assert len(r1) == len(r2) == c["rlen"], (name, c["tag"])
                assert (hashlib.md5(r1.encode("latin1")).hexdigest(), hashlib.md5(r2.encode("latin1")).hexdigest()) == (c["r1_md5"], c["r2_md5"]), (name, c["tag"])
            assert sum(w >> 4 for w in words if w & 15 in (EQ, NE, INS)) == r["end_i"] - st[0] == st[2] + st[3] + st[4]
            assert sum(w >> 4 for w in words if w & 15 in (EQ, NE, DEL, SKIP)) == r["end_j"] - st[1] == st[2] + st[3] + st[5] + st[6]
            assert all((a & 15) != (b & 15) for a, b in zip(words, words[1:]))
            if c["use_jump"]:
                nskip_runs += sum(w & 15 == SKIP for w in words)
            else:
                assert st[6] == 0
            # the M flavour: the same columns, '=' and 'X' merged
            rc, ncm, wm, stm = _host(bytes(r["ops"]), s1, r["end_i"], s2, r["end_j"], extended=False)
            assert rc == 0 and stm == st and sum(w >> 4 for w in wm[:ncm]) == sum(w >> 4 for w in words)
            ncases += 1
    assert ncases > 120
    assert nskip_runs >= 1          # fit -s: the jump state is the spliced gap N


def test_cigar_argument_checks():
    lib = A.load_library()
    ok = (bytes([0, 1, 2]), b"ACG", 2, b"ACG", 2)
    assert _host(*ok)[0] == 0
    # inconsistent lists: a code above 3; more row ops than end_i; more column ops than end_j
    for ops, s1, end_i, s2, end_j in ((bytes([0, 4, 0]), b"ACG", 3, b"ACG", 3), (bytes([0, 1, 1]), b"ACG", 2, b"ACG", 3),
                                      (bytes([3, 3]), b"ACG", 3, b"ACG", 1), (bytes([0]), b"ACG", 0, b"ACG", 3)):
        for want_words in (True, False):
            rc, nc, words, stats = _host(ops, s1, end_i, s2, end_j, want_words=want_words)
            assert (rc, nc, stats) == (A.ERR_DOMAIN, -1, [-1] * 8), ops
            assert _cigar_ref(ops, s1, end_i, s2, end_j) is None
    assert A.ERR_DOMAIN == -4 and A.ERR_ARG == -1
    with pytest.raises(A.AlignToolsError) as e:
        A.cigar(bytes([4]), b"A", 1, b"A", 1)
    assert e.value.code == A.ERR_DOMAIN
    st, nc, w = (C.c_int32 * 8)(), C.c_int32(0), (C.c_uint32 * 4)()
    assert lib.at_cigar(b"\0", -1, b"A", 1, b"A", 1, 0, w, C.byref(nc), st) == A.ERR_ARG
    assert lib.at_cigar(b"\0", 1, b"A", -1, b"A", 1, 0, w, C.byref(nc), st) == A.ERR_ARG
    assert lib.at_cigar(b"\0", 1, b"A", 1, b"A", -1, 0, w, C.byref(nc), st) == A.ERR_ARG
    assert lib.at_cigar(None, 1, b"A", 1, b"A", 1, 0, w, C.byref(nc), st) == A.ERR_ARG
    assert lib.at_cigar(b"\0", 1, None, 1, b"A", 1, 0, w, C.byref(nc), st) == A.ERR_ARG
    assert lib.at_cigar(b"\0", 1, b"A", 1, None, 1, 0, w, C.byref(nc), st) == A.ERR_ARG
    assert lib.at_cigar(b"\0", 1, b"A", 1, b"A", 1, 0, w, None, st) == A.ERR_ARG
    assert lib.at_cigar(b"\0", 1, b"A", 1, b"A", 1, 0, w, C.byref(nc), None) == A.ERR_ARG
    assert lib.at_cigar(None, 0, None, 0, None, 0, 0, None, C.byref(nc), st) == 0 and nc.value == 0 and list(st) == [0] * 8
    # the device and host-buffer entries refuse a NULL handle before they touch a GPU
    assert lib.at_cigar_batch_device(None, 1, *([None] * 1), 2, *([None] * 7), 0, *([None] * 4), 0, None) == -1
    assert b"NULL handle" in lib.at_last_error(None)
    assert lib.at_align_batch_cigar(None, A.MODE_LOCAL, 1, *([None] * 5), 0, *([None] * 8), 0) == -1
    assert b"NULL handle" in lib.at_last_error(None)
    for name in ("at_cigar", "at_cigar_batch_device", "at_align_batch_cigar"):
        assert name in A.ABI_SYMBOLS and getattr(lib, name) is not None


# ---------------------------------------------------------------- GPU half

@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    yield a
    a.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _pair_of_classes(rng, classes, alphabet, inside):
    """A pair whose alignment has the given column classes (END -> START): (ops, s1, end_i, s2, end_j).  len1 / len2 are the rows /
    columns the list consumes, with the end cell at the corner, or, with `inside`, a few bases before the end of the sequences."""
    a, b, ops = [], [], []
    for c in classes:
        x = rng.choice(alphabet)
        y = x if c == EQ else rng.choice([z for z in alphabet if z != x])
        if c in (EQ, NE):
            a.append(x), b.append(y), ops.append(0)
        elif c == INS:
            a.append(x), ops.append(1)
        else:
            b.append(x), ops.append(2 if c == DEL else 3)
    end_i, end_j = len(a), len(b)
    tail = rng.randint(1, 3) if inside else 0
    s1 = bytes(reversed(a)) + bytes(rng.choices(alphabet, k=tail))
    s2 = bytes(reversed(b)) + bytes(rng.choices(alphabet, k=tail))
    return bytes(ops), s1, end_i, s2, end_j


def _patterns(rng, n, W, alphabet):
    """the five shapes of a list of n ops for group width W"""
    cyc = (EQ, INS, NE, DEL, SKIP)                     # (no '=' beside 'X': neighbours differ in both flavours)
    shapes = [[EQ] * n,                                                    # one run carried over every pass
              [cyc[p % 5] for p in range(n)],                              # a new class at every op: ncigar == nops
              [cyc[(p // W) % 5] for p in range(n)],                       # boundaries exactly at multiples of W
              [cyc[((p + 1) // W) % 5] for p in range(n)]]                 # a run that begins on the last lane of a pass
    out = [_pair_of_classes(rng, s, alphabet, inside=k % 2 == 1) for k, s in enumerate(shapes)]
    out.append(_synth_pair(rng, n, alphabet[:2], (12, 1, 1, 1)))           # two letters: long '=' runs
    return out


class _Batch:
    def __init__(self, cases, bits, refuse=()):
        """refuse: indices of pairs that go up with nops = -1"""
        n = len(cases)
        self.n, self.bits, self.cases = n, bits, cases
        words, woff1, woff2, _l1, _l2, got = A.pack_pairs([(c[1], c[3]) for c in cases], bits=bits)
        assert got == bits
        nops = np.array([-1 if k in refuse else len(c[0]) for k, c in enumerate(cases)], dtype=np.int32)
        ops_off = np.zeros(n, dtype=np.int64)
        at = 3
        for k, c in enumerate(cases):
            ops_off[k] = at
            at += len(c[0]) + 1 + k % 3
        ops = np.full(at + 64, 0xee, dtype=np.uint8)                   # (0xee between the lists: not an op)
        for k, c in enumerate(cases):
            ops[ops_off[k]:ops_off[k] + len(c[0])] = np.frombuffer(c[0], dtype=np.uint8)
        self.host = {"words": words.view(np.int32), "woff1": woff1, "woff2": woff2, "ops": ops, "ops_off": ops_off, "nops": nops,
                     "end_i": np.array([c[2] for c in cases], dtype=np.int32), "end_j": np.array([c[4] for c in cases], dtype=np.int32)}
        self.d = {k: _dev(v) for k, v in self.host.items()}
        self.refuse = set(refuse)

    def expected(self, extended):
        """per pair (ncigar, words, stats) from at_cigar"""
        out = []
        for k, c in enumerate(self.cases):
            rc, nc, words, stats = _host(*c, extended=extended)
            if k in self.refuse:
                nc, words, stats = -1, [], [-1] * 8
            else:
                assert rc == (0 if nc >= 0 else A.ERR_DOMAIN)
            out.append((nc, words[:max(nc, 0)], stats))
        return out

    def run(self, al, extended, cap=None, with_stats=True):
        import torch
        d, n = self.d, self.n
        dev = d["ops"].device
        total = sum(max(len(c[0]), 0) for c in self.cases) + 16
        cap = total if cap is None else cap
        d_nc = torch.full((n + 2,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        d_st = torch.full((8 * n + 8,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        d_off = torch.full((n + 3,), 0x5a5a5a5a, dtype=torch.int64, device=dev)
        d_cg = torch.full((total + 16,), FILL, dtype=torch.int32, device=dev)
        al.cigar_batch_device(n, d["words"].data_ptr(), self.bits, d["woff1"].data_ptr(), d["woff2"].data_ptr(), d["end_i"].data_ptr(),
                              d["end_j"].data_ptr(), d["ops"].data_ptr(), d["ops_off"].data_ptr(), d["nops"].data_ptr(),
                              d_nc.data_ptr(), d_st.data_ptr() if with_stats else None, d_off.data_ptr(), d_cg.data_ptr(), cap,
                              extended=extended, stream=_stream())
        torch.cuda.synchronize()
        for k, v in self.host.items():                                 # inputs are only read
            assert np.array_equal(d[k].cpu().numpy(), v), k
        nc, st, off, cg = d_nc.cpu().numpy(), d_st.cpu().numpy(), d_off.cpu().numpy(), d_cg.cpu().numpy().view(np.uint32)
        assert (nc[n:] == 0x5a5a5a5a).all() and (st[8 * n:] == 0x5a5a5a5a).all() and (off[n + 1:] == 0x5a5a5a5a).all()
        if not with_stats:
            assert (st == 0x5a5a5a5a).all()
        return nc[:n], st[:8 * n].reshape(n, 8), off[:n + 1], cg

    def check(self, al, extended, cap=None, ctx=()):
        want = self.expected(extended)
        nc, st, off, cg = self.run(al, extended, cap)
        cap = len(cg) if cap is None else cap
        assert nc.tolist() == [w[0] for w in want], ctx
        assert st.tolist() == [w[2] for w in want], ctx
        assert off.tolist() == np.concatenate(([0], np.cumsum([max(w[0], 0) for w in want]))).tolist(), ctx   # the exclusive scan
        image = np.full(len(cg), FILL, dtype=np.uint32)
        nwritten = 0
        for k, w in enumerate(want):
            if w[0] > 0 and off[k] + w[0] <= cap:
                image[off[k]:off[k] + w[0]] = w[1]
                nwritten += 1
        if not np.array_equal(cg, image):
            for k, w in enumerate(want):
                o = int(off[k])
                assert cg[o:o + max(w[0], 0)].tolist() == image[o:o + max(w[0], 0)].tolist(), (ctx, "pair", k, "nops", len(self.cases[k][0]))
            raise AssertionError((ctx, "words outside every written range changed", np.nonzero(cg != image)[0][:8].tolist()))
        return nwritten


@pytest.mark.gpu
@pytest.mark.parametrize("W", [16, 64])
@pytest.mark.parametrize("bits", [2, 8])
def test_cigar_kernel_pass_boundaries(al, monkeypatch, bits, W):
    """Lists on both sides of every pass boundary in all five shapes, both flavours, in batches of 1, 3, 5, 67 and all pairs -- none
    a multiple of the pairs per wavefront."""
    monkeypatch.setenv("AT_RENDER_GROUP", str(W))
    rng = random.Random(100 * bits + W)
    alphabet = b"ACGT" if bits == 2 else b"LVIKR*"
    cases = []
    for n in (0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W + 1, 200):
        cases += _patterns(rng, n, W, alphabet)
    assert len(cases) == 50
    assert any(len(c[0]) == 200 and _host(*c)[1] == 200 for c in cases) and any(len(c[0]) == 200 and _host(*c)[1] == 1 for c in cases)
    rng.shuffle(cases)
    ncmp = 0
    for extended in (True, False):
        ncmp += _Batch(cases, bits).check(al, extended, ctx=("all", bits, W, extended))
        for npairs in (1, 3, 5, 67):
            sub = [cases[rng.randrange(50)] for _ in range(npairs)]
            ncmp += _Batch(sub, bits).check(al, extended, ctx=(npairs, bits, W, extended))
    nc, st, off, cg = _Batch(cases[:5], bits).run(al, True, with_stats=False)       # no statistics wanted
    assert off[5] == sum(nc)
    print("cigar kernel bits=%d W=%d: %d CIGARs compared" % (bits, W, ncmp))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [16, 64])
def test_cigar_kernel_capacity_and_refused_pairs(al, monkeypatch, W):
    monkeypatch.setenv("AT_RENDER_GROUP", str(W))
    rng = random.Random(W)
    cases = [_synth_pair(rng, rng.choice((0, 3, W, 2 * W + 1, 40)), b"ACGT") for _ in range(21)]
    b = _Batch(cases, 2)
    want = b.expected(True)
    ends = np.cumsum([w[0] for w in want])
    total = int(ends[-1])
    # the capacity cuts the batch in the middle of a pair: that pair and all behind it are not written, the total is complete
    cut = next(k for k in range(8, 21) if want[k][0] > 1)
    for cap in (int(ends[cut]) - 1, int(ends[cut]), 0, total):
        nwritten = b.check(al, True, cap=cap, ctx=("cap", W, cap))
        assert nwritten == sum(1 for k, w in enumerate(want) if w[0] > 0 and ends[k] <= cap)
        assert b.run(al, True, cap=cap)[2][21] == total
    # refused pairs among good neighbours: nops = -1, an op code 4, more row ops than end_i, more column ops than end_j
    bad = list(cases)
    o = bytearray(bad[4][0] or b"\0\0")
    o[len(o) // 2] = 4
    bad[4] = (bytes(o),) + bad[4][1:]
    bad[9] = (bytes([1]) * (bad[9][2] + 1),) + bad[9][1:]
    bad[10] = (bytes([0]) * W + bytes([3]) * (bad[10][4] + 1),) + bad[10][1:]
    for flavour in (True, False):
        bb = _Batch(bad, 2, refuse=(2, 20))
        wantb = bb.expected(flavour)
        assert [k for k, w in enumerate(wantb) if w[0] < 0] == [2, 4, 9, 10, 20]
        assert all(w[2] == [-1] * 8 for w in wantb if w[0] < 0)
        bb.check(al, flavour, ctx=("refused", W, flavour))
    # no pairs at all: only cigar_off[0] = 0 is written
    import torch
    d_off = torch.full((2,), 77, dtype=torch.int64, device="cuda:0")
    al.cigar_batch_device(0, None, 2, None, None, None, None, None, None, None, None, None, d_off.data_ptr(), None, 0, stream=_stream())
    torch.cuda.synchronize()
    assert d_off.cpu().tolist() == [0, 77]


_E2E = [("global", False, b"ACGT"), ("local", False, b"ACGT"), ("fit", False, b"ACGT"), ("fit", True, b"ACGT"), ("overlap", False, b"ACGT"),
        ("local", False, b"ARNDCQEGHILKMFPSTWYV"), ("global", False, b"ACGTN")]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,jump,alphabet", _E2E, ids=["%s%s-%d" % (m, "-s" if j else "", len(a)) for m, j, a in _E2E])
def test_align_batch_cigar_equals_host_cigar_of_the_ops(al, mode, jump, alphabet):
    rng = random.Random(len(mode) * 7 + jump + len(alphabet))
    pairs = []
    for k in range(62):
        l1 = rng.choice((149, 150, 151)) if k % 10 == 9 else rng.randint(1, 70)
        l2 = rng.choice((149, 150, 151)) if k % 10 == 9 else rng.randint(1, 70)
        if mode == "fit":
            l1, l2 = min(l1, l2), max(l1, l2)
        a = bytes(rng.choices(alphabet, k=l1))
        b = bytearray(rng.choices(alphabet, k=l2))
        if k % 3:                                                       # related pairs: long '=' runs, a few gaps
            src = a if rng.random() < 0.7 or len(a) < 8 else a[:len(a) // 2] + a[len(a) // 2 + 3:]
            at = rng.randint(0, max(0, l2 - len(src)))
            b[at:at + len(src)] = src[:l2 - at]
            b = b[:l2]
        pairs.append((a, bytes(b)))
    al.set_scoring(use_jump=jump, sites=[5, 20, 21, 40, 66, 100, 120] if jump else None)
    try:
        ref = al.align_batch(mode, pairs, render=False)
        nruns = 0
        for extended in (True, False):
            got = al.align_batch_cigar(mode, pairs, extended=extended)
            assert "[cigar: 16 lanes per pair]" in al.last_config
            for name in ("score", "end_i", "end_j", "state"):
                assert np.array_equal(got[name], ref[name]), name
            assert got["cigar_off"].tolist() == np.concatenate(([0], np.cumsum(got["ncigar"]))).tolist()
            for k, (a, b) in enumerate(pairs):
                rc, nc, words, stats = _host(ref["ops"][k], a, int(ref["end_i"][k]), b, int(ref["end_j"][k]), extended)
                assert rc == 0 and got["ncigar"][k] == nc and got["cigar"][k].tolist() == words[:nc], (mode, k, extended)
                assert got["stats"][k].tolist() == stats, (mode, k)
                nruns += nc
        assert nruns > len(pairs)                       # (not vacuous: more than one run per pair over the two flavours)
    finally:
        al.set_scoring()


@pytest.mark.gpu
def test_align_batch_cigar_chunked_host_path(al, monkeypatch):
    """2 x AT_HOST_CHUNK_MIN pairs of 36 bases: the chunks' payloads land back to back in pair order"""
    monkeypatch.setenv("AT_HOST_CHUNK_MIN", "1024")
    rng = random.Random(36)
    n = 2048
    reads = [bytes(rng.choices(b"ACGT", k=36)) for _ in range(n)]
    pairs = []
    for a in reads:
        b = bytearray(a)
        for _ in range(rng.randint(0, 4)):
            b[rng.randrange(36)] = rng.choice(b"ACGT")
        if rng.random() < 0.3:
            del b[rng.randrange(30)]
            b.append(rng.choice(b"ACGT"))
        pairs.append((a, bytes(b)))
    got = al.align_batch_cigar("local", pairs)
    assert " x2 chunks" in al.last_config and "[cigar: 16 lanes per pair]" in al.last_config, al.last_config
    ref = al.align_batch("local", pairs, render=False)
    assert np.array_equal(got["score"], ref["score"]) and np.array_equal(got["end_i"], ref["end_i"]) and np.array_equal(got["end_j"], ref["end_j"])
    assert (got["ncigar"] > 0).all()
    assert got["cigar_off"].tolist() == np.concatenate(([0], np.cumsum(got["ncigar"]))).tolist()      # contiguous across the chunks
    for k in sorted(rng.sample(range(n), 496) + [0, 1023, 1024, n - 1]):
        rc, nc, words, stats = _host(ref["ops"][k], pairs[k][0], int(ref["end_i"][k]), pairs[k][1], int(ref["end_j"][k]))
        assert rc == 0 and got["cigar"][k].tolist() == words[:nc] and got["stats"][k].tolist() == stats, k
    # a buffer that ends in the middle of the second chunk: offsets and counts complete, the pairs that fit written, nothing behind
    lib = A.load_library()
    blob, off1, len1, off2, len2 = A._flatten(pairs)
    kcut = next(k for k in range(1500, n) if got["ncigar"][k] > 1)
    cap = int(got["cigar_off"][kcut]) + 1
    score, ei, ej, st, nc = (np.zeros(n, dtype=np.int32) for _ in range(5))
    stats = np.zeros((n, 8), dtype=np.int32)
    off = np.zeros(n + 1, dtype=np.int64)
    words = np.full(int(got["cigar_off"][n]) + 8, FILL, dtype=np.uint32)
    ptr = A._ptr
    assert lib.at_align_batch_cigar(al._h, A.MODE_LOCAL, n, ptr(blob), ptr(off1), ptr(len1), ptr(off2), ptr(len2), 0, ptr(score), ptr(ei),
                                    ptr(ej), ptr(st), ptr(stats), ptr(nc), ptr(off), ptr(words), cap) == 0
    assert np.array_equal(off, got["cigar_off"]) and np.array_equal(nc, got["ncigar"]) and np.array_equal(stats, got["stats"])
    full = np.concatenate(got["cigar"])
    assert np.array_equal(words[:off[kcut]], full[:off[kcut]]) and (words[off[kcut]:] == FILL).all()


def _many_run_pairs(rng, n, length):
    """pairs whose global alignment changes class every few columns: every third base substituted, so some thirty runs per pair"""
    pairs = []
    for _ in range(n):
        a = bytes(rng.choices(b"ACGT", k=length))
        b = bytearray(a)
        for p in range(rng.randrange(3), length, 3):
            b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + rng.randrange(3)) % 4]
        pairs.append((a, bytes(b)))
    return pairs


@pytest.mark.gpu
def test_align_batch_cigar_more_runs_than_the_first_guess():
    """More than 16 runs per pair: Aligner.align_batch_cigar's first buffer (16 n + 64 words) is too small and it calls again; on
    a fresh handle the batch also has more words than the host entry fetches unasked, so the rest comes down behind the total."""
    rng = random.Random(33)
    pairs = _many_run_pairs(rng, 1000, 60)
    al = A.Aligner()
    try:
        got = al.align_batch_cigar("global", pairs)
        ref = al.align_batch("global", pairs, render=False)
    finally:
        al.close()
    total = int(got["cigar_off"][-1])
    assert total > 16 * len(pairs) + 64 and total > 1.25 * 4.0 * len(pairs) + 16384
    assert got["cigar_off"].tolist() == np.concatenate(([0], np.cumsum(got["ncigar"]))).tolist()
    assert np.array_equal(got["score"], ref["score"])
    for k, (a, b) in enumerate(pairs):
        rc, nc, words, stats = _host(ref["ops"][k], a, int(ref["end_i"][k]), b, int(ref["end_j"][k]))
        assert rc == 0 and got["cigar"][k].tolist() == words[:nc] and got["stats"][k].tolist() == stats, k
