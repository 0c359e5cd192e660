"""`alignTools batch fit --long-targets --queries q.fa (--score-only | --paf) genome.fa`: end-to-end affine alignment of reads against
long targets (at_scan_fit), in the output form that `batch local --long-targets` has.

The refusals run anywhere.  On the GPU the expected output is built from Aligner.scan_fit, as tests/test_cli_scan_local.py builds its
lines from the Python API, and compared byte for byte with the binary's."""
import os
import random
import subprocess

import pytest

import aligntools.c_amd as A
from conftest import ROOT

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")
BASE = ["batch", "fit", "-m", "2", "-u", "-2", "-o", "-5", "-e", "-2"]


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("argv,why", [
    (BASE + ["-s", "--long-targets", "--queries", "q.fa", "--score-only", "t.fa"], b"fit --long-targets does not go with -s (jump sites are per-target columns)\n"),
    (BASE + ["--long-targets", "--score-only", "t.fa"], b"--long-targets goes with --queries (reads against long targets)\n"),
    (BASE + ["--long-targets", "--all-vs-all", "--queries", "q.fa", "--score-only", "t.fa"], b"--long-targets does not go with --all-vs-all\n"),
    (BASE + ["--long-targets", "--queries", "q.fa", "--gpus", "2", "--score-only", "t.fa"], b"--long-targets runs on one GPU: it does not go with --gpus N > 1\n"),
    (BASE + ["--long-targets", "--scan", "--queries", "q.fa", "--score-only", "t.fa"], b"--long-targets does not go with --scan, --infix or --keep\n"),
    (BASE + ["--long-targets", "--keep", "5", "--queries", "q.fa", "--score-only", "t.fa"], b"--long-targets does not go with --scan, --infix or --keep\n"),
    (BASE + ["--long-targets", "--queries", "q.fa", "t.fa"], b"--long-targets needs one of --score-only and --paf\n"),
    (BASE + ["--long-targets", "--queries", "q.fa", "--score-only", "--paf", "t.fa"], b"--long-targets needs one of --score-only and --paf\n"),
    (["batch", "global", "--long-targets", "--queries", "q.fa", "--score-only", "t.fa"], b"--long-targets goes with local\n"),
    (["batch", "overlap", "--long-targets", "--queries", "q.fa", "--score-only", "t.fa"], b"--long-targets goes with local\n"),
    (["batch", "edit", "-u", "1", "--long-targets", "--queries", "q.fa", "--score-only", "t.fa"], b"--long-targets goes with local\n"),
], ids=["sites", "no-queries", "all-vs-all", "gpus", "scan", "keep", "no-format", "both-formats", "global", "overlap", "edit"])
def test_cli_fit_long_targets_refusals(built, tmp_path, argv, why):
    """Refused with a message, the usage text and return code 1 before any GPU call (the files need not exist)"""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(why + b"Usage:"), p.stderr
    lines = [ln for ln in p.stderr.split(b"\n") if b"alignTools batch" in ln]
    assert len(lines) == 2 and b"[--long-targets]" not in lines[0] and lines[1].count(b"[--long-targets]") == 1


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """six reads against a 6 000-base target among short ones (one shorter than most reads); reads planted as given and
    reverse-complemented, with edits"""
    d = tmp_path_factory.mktemp("scan_fit")
    rng = random.Random(47)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    queries = [rnd(rng.randint(60, 150)) for _ in range(6)]
    queries[2] = "ACGT" * 16                                            # its own reverse complement
    big = list(rnd(6000))
    for k, at in ((0, 700), (1, 4090), (3, 5800)):
        body = queries[k] if k != 1 else A.revcomp(queries[k]).decode()
        body = body[:20] + rnd(1) + body[21:50] + body[52:]                # a substitution and a deletion
        big[at:at + len(body)] = body
    targets = [rnd(50), "".join(big), queries[4][:-2] + rnd(230), rnd(300) + A.revcomp(queries[5]).decode() + rnd(11), "ACGT" * 40]
    qn, tn = ["q%d" % k for k in range(6)], ["t%d" % k for k in range(5)]
    for name, names, seqs in (("q.fa", qn, queries), ("t.fa", tn, targets)):
        with open(d / name, "w") as fh:
            for n, s in zip(names, seqs):
                fh.write(">%s\n%s\n" % (n, s))
    return d, qn, queries, tn, targets


def _lines(qn, queries, tn, targets, both, k, min_score):
    al = A.Aligner()
    try:
        al.set_scoring(2, -2, -5, -2, -10)
        r = al.scan_fit(queries, targets, k=k, min_score=min_score, strands="both" if both else "forward", cigar=True)
    finally:
        al.close()
    plain, paf = [], []
    for q in range(len(queries)):
        for j in range(int(r["nhits"][q])):
            t, score, end_i, end_j = (int(r[name][q, j]) for name in ("target", "score", "end_i", "end_j"))
            s = "-" if both and r["strand"][q, j] == 1 else "+"
            plain.append("%s\t%s\tscore=%f%s\n" % (qn[q], tn[t], score, "\t" + s if both else ""))      # (the hit line of `batch fit --queries`)
            st = [int(x) for x in r["stats"][q, j]]
            ql = len(queries[q])
            qs, qe = (st[0], end_i) if s == "+" else (ql - end_i, ql - st[0])
            cols = [qn[q], ql, qs, qe, s, tn[t], len(targets[t]), st[1], end_j, st[2], st[2] + st[3] + st[4] + st[5], 255]
            line = "\t".join(str(c) for c in cols) + "\tAS:i:%d\tNM:i:%d" % (score, st[3] + st[4] + st[5])
            if len(r["cigar"][q][j]):
                line += "\tcg:Z:" + A.cigar_string(r["cigar"][q][j]).decode()
            paf.append(line + "\n")
    return plain, paf


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True], ids=["forward", "both-strands"])
def test_cli_fit_long_targets_output(built, files, both):
    d, qn, queries, tn, targets = files
    plain, paf = _lines(qn, queries, tn, targets, both, 3, None)
    assert len(plain) == 18 and any(int(x.split("\t")[7]) > 4000 for x in paf) and not any("\tt0\t" in x for x in plain)
    assert all(x.split("\t")[2:4] == ["0", x.split("\t")[1]] for x in paf)          # fit takes the whole read
    if both:
        assert {"+", "-"} == {x.split("\t")[4] for x in paf}
    argv = [EXE] + BASE + ["--long-targets", "--queries", "q.fa", "--best", "3"] + (["--both-strands"] if both else [])
    p = subprocess.run(argv + ["--score-only", "t.fa"], cwd=d, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == plain
    p = subprocess.run(argv + ["--paf", "t.fa"], cwd=d, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf
    # --min-score is the cutoff
    plain, _paf = _lines(qn, queries, tn, targets, both, 3, 60)
    assert 0 < len(plain) < 18
    p = subprocess.run(argv + ["--min-score", "60", "--score-only", "t.fa"], cwd=d, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == plain
