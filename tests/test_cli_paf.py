"""`alignTools batch <global|local|fit|overlap> ... --paf`: one PAF line per pair / hit instead of the name line and the two strings.

The refusals run anywhere.  On the GPU the lines are built here from Aligner.search + Aligner.align_batch and the restatement of the
CIGAR rule in test_cigar.py, and compared line for line with the binary's output; without --paf the same invocations must print
the name lines and strings they always printed."""
import os
import random
import subprocess

import pytest

import aligntools.c_amd as A
from conftest import ROOT
from test_cigar import _cigar_ref

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")
SITES = " 7|30|31|60|95|140"
SITE_LIST = [7, 30, 31, 60, 95, 140]


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("argv,why", [
    (["batch", "edit", "--paf", "p.fa"], b"--paf does not go with edit"),
    (["batch", "local", "--paf", "--score-only", "p.fa"], b"--paf does not go with --score-only"),
    (["batch", "overlap", "--all-vs-all", "--paf", "p.fa"], b"--paf does not go with --all-vs-all"),
    (["batch", "global", "--gpus", "2", "--paf", "p.fa"], b"--paf runs on one GPU: it does not go with --gpus N > 1"),
    (["batch", "edit", "--queries", "q.fa", "--paf", "t.fa"], b"--paf does not go with edit"),
    (["batch", "local", "--queries", "q.fa", "--best", "3", "--score-only", "--paf", "t.fa"], b"--paf does not go with --score-only"),
], ids=["edit", "score-only", "all-vs-all", "gpus", "queries-edit", "queries-score-only"])
def test_cli_paf_refusals(built, tmp_path, argv, why):
    """Refused with a message, the usage line and return code 1 before any GPU call (the files need not exist)."""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(why), p.stderr
    assert b"Usage:" in p.stderr and b"[--paf]" in p.stderr
    assert b"--queries <queries.fa> [--best K] [--both-strands]" in p.stderr


def test_cli_usage_line_keeps_its_parts(built, tmp_path):
    p = subprocess.run([EXE, "batch", "local", "--best", "2", "p.fa"], cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stderr.startswith(b"--best goes with --queries")
    p = subprocess.run([EXE, "batch", "local", "--min-score", "2", "p.fa"], cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stderr.startswith(b"--min-score goes with ")
    assert p.stderr.count(b"[--paf]") == 2


# ---------------------------------------------------------------- GPU

def _write(path, names, seqs, comments=None):
    with open(path, "w") as fh:
        for k, (n, s) in enumerate(zip(names, seqs)):
            fh.write(">%s%s\n%s\n" % (n, (comments or {}).get(k, ""), s))


def _paf(qn, ql, strand, tn, tl, score, end_i, end_j, words, st):
    qs, qe = (st[0], end_i) if strand == "+" else (ql - end_i, ql - st[0])
    cols = [qn, ql, qs, qe, strand, tn, tl, st[1], end_j, st[2], st[2] + st[3] + st[4] + st[5], 255]
    line = "\t".join(str(c) for c in cols) + "\tAS:i:%d\tNM:i:%d" % (score, st[3] + st[4] + st[5])
    if words:
        line += "\tcg:Z:" + "".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in words)
    return line + "\n"


def _expected(al, mode, items):
    """items: (qname, query as in the file, strand, tname, target).  Returns (PAF lines, the records printed without --paf)."""
    pairs = [(A.revcomp(q) if s == "-" else q.encode(), t.encode()) for _qn, q, s, _tn, t in items]
    r = al.align_batch(mode, pairs)
    paf, plain = [], []
    for k, (qn, q, s, tn, t) in enumerate(items):
        words, st = _cigar_ref(r["ops"][k], pairs[k][0], int(r["end_i"][k]), pairs[k][1], int(r["end_j"][k]))
        paf.append(_paf(qn, len(q), s, tn, len(t), int(r["score"][k]), int(r["end_i"][k]), int(r["end_j"][k]), words, st))
        plain.append((qn, tn, "score=%d.000000" % r["score"][k], r["r1"][k], r["r2"][k]))
    return paf, plain


@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    yield a
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cmd,flags", [("local", []), ("fit", ["-s"])], ids=["local", "fit-s"])
@pytest.mark.parametrize("both", [False, True], ids=["forward", "both-strands"])
def test_cli_paf_search(built, al, tmp_path, cmd, flags, both):
    rng = random.Random(len(cmd) + 2 * both)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    queries = [rnd(rng.randint(20, 40)) for _ in range(7)]
    queries[3] = "ACGT" * 6                                            # its own reverse complement: + and - tie on every target
    targets = []
    for t in range(5):
        q = queries[(2 * t) % 7]
        if t % 2:
            q = A.revcomp(q).decode()
        q = q[:10] + rnd(1) + q[11:14] + q[16:]                        # a mismatch (perhaps) and a gap
        targets.append((rnd(rng.randint(3, 12)) + q + rnd(20))[:60].ljust(40, "A"))
    assert all(20 <= len(x) <= 60 for x in queries + targets)
    qn = ["q%d" % k for k in range(7)]
    tn = ["t%d" % k for k in range(5)]
    _write(tmp_path / "q.fa", qn, queries)
    _write(tmp_path / "t.fa", tn, targets, {0: SITES} if flags else None)
    al.set_scoring(use_jump=bool(flags), sites=SITE_LIST if flags else None)
    try:
        hits = al.search(cmd, queries, targets, k=3, strands="both" if both else "forward")
        items = []
        for q in range(7):
            for j in range(int(hits["nhits"][q])):
                t = int(hits["target"][q, j])
                items.append((qn[q], queries[q], "-" if both and hits["strand"][q, j] == 1 else "+", tn[t], targets[t]))
        paf, plain = _expected(al, cmd, items)
    finally:
        al.set_scoring()
    assert len(items) == 21
    argv = [EXE, "batch", cmd] + flags + ["--queries", "q.fa", "--best", "3"] + (["--both-strands"] if both else [])
    p = subprocess.run(argv + ["--paf", "t.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.decode().splitlines(keepends=True)
    assert got == paf
    assert all(len(line.split("\t")) in (14, 15) and line.split("\t")[11] == "255" for line in got)
    if both:
        strands = [(line.split("\t")[0], line.split("\t")[5], line.split("\t")[4]) for line in got]
        assert any(a[:2] == b[:2] == ("q3", a[1]) and (a[2], b[2]) == ("+", "-") for a, b in zip(strands, strands[1:]))
        assert {"+", "-"} == {s[2] for s in strands}
    # without --paf: the name lines and strings as always
    p = subprocess.run(argv + ["t.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    want = "".join("%s\t%s\t%s%s\n%s\n%s\n" % (a, b, sc, "\t" + it[2] if both else "", r1, r2) for (a, b, sc, r1, r2), it in zip(plain, items))
    assert p.stdout.decode() == want


@pytest.mark.gpu
@pytest.mark.parametrize("cmd", ["global", "local", "fit", "overlap"])
def test_cli_paf_pair_file(built, al, tmp_path, cmd):
    rng = random.Random(len(cmd))
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    items = []
    for k in range(9):
        a = rnd(rng.randint(1, 50))
        b = (rnd(rng.randint(0, 9)) + a[:len(a) // 2] + rnd(k % 3) + a[len(a) // 2 + k % 2:] + rnd(rng.randint(0, 9))) if k % 4 else rnd(rng.randint(1, 60))
        if cmd == "fit" and len(a) > len(b):
            a, b = b, a
        items.append(("a%d" % k, a, "+", "b%d" % k, b))
    with open(tmp_path / "p.fa", "w") as fh:
        for qn, q, _s, tn, t in items:
            fh.write(">%s\n%s\n>%s\n%s\n" % (qn, q, tn, t))
    paf, plain = _expected(al, cmd, items)
    p = subprocess.run([EXE, "batch", cmd, "--paf", "p.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf
    assert b"[main] CMD:" in p.stderr
    p = subprocess.run([EXE, "batch", cmd, "p.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("%s\t%s\t%s\n%s\n%s\n" % rec for rec in plain)


@pytest.mark.gpu
def test_cli_paf_more_runs_than_the_first_buffer(built, al, tmp_path):
    """Nine pairs with some thirty runs each: more words than the CLI's first buffer (16 per pair + 64), so it calls again"""
    from test_cigar import _many_run_pairs
    pairs = _many_run_pairs(random.Random(9), 9, 90)
    items = [("a%d" % k, a.decode(), "+", "b%d" % k, b.decode()) for k, (a, b) in enumerate(pairs)]
    with open(tmp_path / "p.fa", "w") as fh:
        for qn, q, _s, tn, t in items:
            fh.write(">%s\n%s\n>%s\n%s\n" % (qn, q, tn, t))
    paf, _plain = _expected(al, "global", items)
    assert sum(line.rsplit("cg:Z:", 1)[1].count("=") + line.rsplit("cg:Z:", 1)[1].count("X") for line in paf) > 16 * 9 + 64
    p = subprocess.run([EXE, "batch", "global", "--paf", "p.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf
