"""`alignTools batch edit -u 1 --infix --scan --all-hits D [--min-sep S] --queries q.fa (--score-only | --paf) genome.fa`: every
occurrence of every read with at most D edits (at_scan_hits).

The refusals run anywhere.  On the GPU the expected output is built from Aligner.scan_hits, as tests/test_cli_scan.py builds its
lines from Aligner.scan, and compared byte for byte with the binary's."""
import os
import random
import subprocess

import pytest

import aligntools.c_amd as A
from conftest import ROOT

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")
BASE = ["batch", "edit", "-u", "1", "--infix"]


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("argv,why", [
    (BASE + ["--all-hits", "3", "--queries", "q.fa", "--score-only", "t.fa"], b"--all-hits goes with --scan\n"),
    (BASE + ["--scan", "--all-hits", "3", "--best", "2", "--queries", "q.fa", "--score-only", "t.fa"],
     b"--all-hits does not go with --best (it reports every occurrence)\n"),
    (BASE + ["--scan", "--min-sep", "10", "--queries", "q.fa", "--score-only", "t.fa"], b"--min-sep goes with --all-hits\n"),
    (BASE + ["--scan", "--all-hits", "-1", "--queries", "q.fa", "--score-only", "t.fa"], b"--all-hits D needs D >= 0\n"),
    (BASE + ["--scan", "--all-hits", "3", "--min-sep", "-2", "--queries", "q.fa", "--paf", "t.fa"],
     b"--min-sep S needs S >= 0 (or -1: each read's own length)\n"),
    (BASE + ["--scan", "--all-hits", "3", "--queries", "q.fa", "t.fa"], b"--scan needs --score-only or --paf\n"),
], ids=["no-scan", "best", "sep-alone", "negative", "sep-below", "no-format"])
def test_cli_all_hits_refusals(built, tmp_path, argv, why):
    """Refused with a message, the usage text and return code 1 before any GPU call (the files need not exist)"""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(why + b"Usage:"), p.stderr
    lines = [ln for ln in p.stderr.split(b"\n") if b"alignTools batch" in ln]
    assert len(lines) == 2 and b"[--all-hits D] [--min-sep S]" in lines[1] and b"--all-hits" not in lines[0]
    assert p.stderr.count(b"[--scan]") == 2 and p.stderr.count(b"[--infix]") == 2 and p.stderr.count(b"[--paf]") == 2


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """five reads against a 7 000-base target among short ones; read 0 at three loci (one with edits), read 1 reverse-complemented
    at two, read 2 its own reverse complement in a tandem"""
    d = tmp_path_factory.mktemp("scanhits")
    rng = random.Random(43)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    queries = [rnd(rng.randint(60, 150)) for _ in range(5)]
    queries[2] = "ACGT" * 12
    big = list(rnd(7000))
    q0 = queries[0]
    for at, body in ((500, q0), (3900, q0[:20] + rnd(1) + q0[21:50] + q0[52:]), (6500, q0)):
        big[at:at + len(body)] = body
    rc1 = A.revcomp(queries[1]).decode()
    for at in (1500, 5000):
        big[at:at + len(rc1)] = rc1
    targets = [rnd(90), "".join(big), queries[3][5:] + rnd(30), "ACGT" * 40]
    qn, tn = ["q%d" % k for k in range(5)], ["t%d" % k for k in range(4)]
    for name, names, seqs in (("q.fa", qn, queries), ("t.fa", tn, targets)):
        with open(d / name, "w") as fh:
            for n, s in zip(names, seqs):
                fh.write(">%s\n%s\n" % (n, s))
    return d, qn, queries, tn, targets


def _lines(qn, queries, tn, targets, both, max_dist, min_sep):
    al = A.Aligner()
    try:
        al.set_scoring(1, 1, -5, -1, -10)
        r = al.scan_hits(queries, targets, max_dist, min_sep=min_sep, strands="both" if both else "forward", cigar=True)
    finally:
        al.close()
    plain, paf = [], []
    for q in range(len(queries)):
        for e in range(int(r["hit_off"][q]), int(r["hit_off"][q + 1])):
            t, dist, end_j = (int(r[name][e]) for name in ("target", "score", "end_j"))
            s = "-" if r["strand"][e] == 1 else "+"
            plain.append("%s\t%s\tedit_distance=%d\tend=%d%s\n" % (qn[q], tn[t], dist, end_j, "\t" + s if both else ""))
            st = [int(x) for x in r["stats"][e]]
            ql = len(queries[q])
            assert st[3] + st[4] + st[5] == dist and st[0] == 0
            cols = [qn[q], ql, 0, ql, s, tn[t], len(targets[t]), st[1], end_j, st[2], st[2] + st[3] + st[4] + st[5], 255]
            line = "\t".join(str(c) for c in cols) + "\tAS:i:%d\tNM:i:%d" % (-dist, dist)
            if len(r["cigar"][e]):
                line += "\tcg:Z:" + A.cigar_string(r["cigar"][e]).decode()
            paf.append(line + "\n")
    return plain, paf


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True], ids=["forward", "both-strands"])
def test_cli_all_hits_output(built, files, both):
    d, qn, queries, tn, targets = files
    plain, paf = _lines(qn, queries, tn, targets, both, 6, -1)
    loci = [int(x.split("\t")[8]) for x in paf if x.startswith("q0\t") and x.split("\t")[5] == "t1"]
    assert len(loci) == 3 and max(loci) > 3792 and len(targets[1]) > 3792             # three loci of one read in one long target
    if both:
        assert {"+", "-"} == {x.split("\t")[4] for x in paf}
        assert sum(x.startswith("q1\tt1\t") and x.endswith("\t-\n") for x in plain) == 2
    argv = [EXE] + BASE + ["--scan", "--all-hits", "6", "--queries", "q.fa"] + (["--both-strands"] if both else [])
    p = subprocess.run(argv + ["--score-only", "t.fa"], cwd=d, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == plain
    p = subprocess.run(argv + ["--paf", "t.fa"], cwd=d, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf
    # --min-sep 0: every occurrence (the tandem read has one every four columns)
    plain0, paf0 = _lines(qn, queries, tn, targets, both, 6, 0)
    assert len(plain0) > len(plain)
    p = subprocess.run(argv + ["--min-sep", "0", "--paf", "t.fa"], cwd=d, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf0
