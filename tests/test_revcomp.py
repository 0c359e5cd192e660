"""at_revcomp / at_revcomp_device: the reverse complement on the host (bytes) and on the device (packed words).

The host helper is held to a table written out here; the device kernel to at_pack_batch on the at_revcomp-ed bytes, word for
word, slack word included, with every other word of the output buffer untouched."""
import ctypes as C
import random

import numpy as np
import pytest

import aligntools.c_amd as A

# the IUPAC complement, upper case; the lower-case letters likewise; every other byte maps to itself
COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "U": "A", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
        "S": "S", "W": "W", "N": "N"}
TABLE = list(range(256))
for _a, _b in COMP.items():
    TABLE[ord(_a)] = ord(_b)
    TABLE[ord(_a.lower())] = ord(_b.lower())


def _py_revcomp(s):
    return bytes(TABLE[c] for c in reversed(s))


@pytest.fixture(scope="module")
def lib():
    from aligntools.c_amd import build
    build.build()
    return A.load_library()


def test_revcomp_every_byte_value(lib):
    for v in range(256):
        assert A.revcomp(bytes([v])) == bytes([TABLE[v]]), v
    every = bytes(range(256))
    assert A.revcomp(every) == _py_revcomp(every)
    assert A.revcomp("ACGTacgt") == b"acgtACGT"


def test_revcomp_lengths_and_involution(lib):
    assert A.revcomp(b"") == b""
    assert A.revcomp(b"A") == b"T" and A.revcomp(b"g") == b"c"
    rng = random.Random(1)
    letters = "ACGTRYKMBVDHSWNacgtrykmbvdhswn"
    for n in (1, 3, 7, 151, 1023):
        s = "".join(rng.choice(letters) for _ in range(n)).encode()
        r = A.revcomp(s)
        assert r == _py_revcomp(s)
        assert A.revcomp(r) == s                                           # (without U: the table is an involution)
    assert A.revcomp(A.revcomp(b"AUG")) == b"ATG"


def test_revcomp_other_bytes_are_reversed_only(lib):
    s = b"EFIJLOPQXZ*-. 0189\x00\xff\x80efijlopqxz"
    assert A.revcomp(s) == s[::-1]


def test_revcomp_bad_arguments(lib):
    out = C.create_string_buffer(8)
    assert lib.at_revcomp(b"ACGT", -1, out) == -1
    assert lib.at_revcomp(None, 4, out) == -1
    assert lib.at_revcomp(None, 0, None) == 0
    assert lib.at_revcomp_device(None, 1, None, 2, None, None, None, None, None) == -1
    assert b"NULL handle" in lib.at_last_error(None)


# ---------------------------------------------------------------- GPU
LENGTHS = list(range(0, 71)) + [149, 150, 151, 1000, 1023, 1024]


@pytest.fixture(scope="module")
def al():
    a = A.Aligner(0)
    yield a
    a.close()


def _pack_reads(reads, bits):
    """The reads as s1 of pairs with an empty s2: words and the word offset of every read (at_pack_batch)."""
    words, woff1, _woff2, len1, _len2, got = A.pack_pairs([(r, b"") for r in reads], bits=bits)
    assert got == bits
    return words, woff1, len1


@pytest.mark.gpu
@pytest.mark.parametrize("bits,alphabet", [(2, "ACGT"), (8, "ACGT"), (8, "ACGTNacgtnRYKMBVDHSWU"), (8, "ACDEFGHIKLMNPQRSTVWY")],
                         ids=["2bit", "8bit-acgt", "8bit-iupac", "8bit-protein"])
@pytest.mark.parametrize("own_offsets", [False, True], ids=["same-offsets", "out-offsets"])
def test_revcomp_device_equals_pack_of_revcomp(al, bits, alphabet, own_offsets):
    import torch
    rng = random.Random(bits * 100 + len(alphabet))
    lens = LENGTHS + [rng.choice(LENGTHS) for _ in range(40)]
    rng.shuffle(lens)
    reads = ["".join(rng.choice(alphabet) for _ in range(n)).encode() for n in lens]
    words, woff, ln = _pack_reads(reads, bits)
    want_words, want_woff, _ = _pack_reads([A.revcomp(r) for r in reads], bits)
    assert np.array_equal(want_woff, woff)
    n = len(reads)
    bpw = 32 // bits
    nw = [(x + bpw - 1) // bpw + 1 for x in lens]
    total = len(words)
    if own_offsets:
        # the output reads in reverse order with 3 words between them and 5 in front
        out_woff = np.zeros(n, dtype=np.int64)
        at = 5
        for r in reversed(range(n)):
            out_woff[r] = at
            at += nw[r] + 3
        total = at + 7
    else:
        out_woff = woff
    pattern = np.uint32(0xDEADBEEF)
    want = np.full(total, pattern, dtype=np.uint32)
    for r in range(n):
        want[out_woff[r]:out_woff[r] + nw[r]] = want_words[woff[r]:woff[r] + nw[r]]
    dev = torch.device("cuda", 0)
    tt = lambda x: torch.from_numpy(x).to(dev)
    d_words, d_woff, d_len = tt(words.view(np.int32)), tt(woff), tt(ln)
    d_out = tt(np.full(total, pattern, dtype=np.uint32).view(np.int32))
    d_out_woff = tt(out_woff) if own_offsets else None
    al.revcomp_device(n, d_words.data_ptr(), bits, d_woff.data_ptr(), d_len.data_ptr(), d_out.data_ptr(),
                      d_out_woff.data_ptr() if own_offsets else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    # (same offsets: the slack words of the empty second sequences lie between the reads and must keep the pattern)
    bad =np.flatnonzero(got != want)
    assert bad.size == 0, (bits, alphabet, bad[:8], [hex(int(got[b])) for b in bad[:8]], [hex(int(want[b])) for b in bad[:8]])
    assert np.array_equal(d_words.cpu().numpy().view(np.uint32), words)     # the input is only read


@pytest.mark.gpu
def test_revcomp_device_argument_checks(al):
    for args in [(-1, 8, 2, 8, 8, 8), (1, 8, 4, 8, 8, 8), (1, 0, 2, 8, 8, 8), (1, 8, 2, 0, 8, 8), (1, 8, 2, 8, 0, 8), (1, 8, 2, 8, 8, 0)]:
        nseq, d_seq, bits, d_woff, d_len, d_out = args
        with pytest.raises(A.AlignToolsError) as ei:
            al.revcomp_device(nseq, d_seq or None, bits, d_woff or None, d_len or None, d_out or None)
        assert ei.value.code == -1
    al.revcomp_device(0, None, 2, None, None, None)                          # nothing to do
