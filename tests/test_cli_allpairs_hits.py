"""`alignTools batch <global|local|overlap|edit> --all-vs-all --keep T (--score-only | --paf) reads.fa`: only the pairs over the
threshold leave the GPU (at_allpairs_hits).

The refusals run anywhere.  On the GPU --score-only is compared with the dense run's lines (for overlap: byte for byte with
--min-score T), and every --paf line is rebuilt from Aligner.allpairs_hits(..., cigar=True)."""
import os
import random
import subprocess

import pytest

import aligntools.c_amd as A
from conftest import ROOT

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")
AVA = ["--all-vs-all", "--keep", "30"]


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


def _usage_counts(stderr):
    lines = [ln for ln in stderr.split(b"\n") if b"alignTools batch" in ln]
    assert len(lines) == 2
    assert b"[--keep T]" in lines[0] and b"--keep" not in lines[1]
    assert b"--queries <queries.fa> [--best K] [--both-strands]" in lines[1]
    for flag in (b"[--paf]", b"[--alignments]", b"[--infix]"):
        assert stderr.count(flag) == 2, flag


@pytest.mark.parametrize("argv,why", [
    (["batch", "overlap", "--keep", "30", "--score-only", "r.fa"], b"--keep goes with --all-vs-all\n"),
    (["batch", "overlap"] + AVA + ["--queries", "q.fa", "--score-only", "r.fa"],
     b"--keep does not go with --queries (it keeps pairs of --all-vs-all)\n"),
    (["batch", "overlap"] + AVA + ["--gpus", "2", "--score-only", "r.fa"], b"--keep runs on one GPU: it does not go with --gpus N > 1\n"),
    (["batch", "overlap"] + AVA + ["--min-score", "30", "--score-only", "r.fa"], b"--keep does not go with --min-score (it is the threshold)\n"),
    (["batch", "edit", "-u", "1", "--infix"] + AVA + ["--score-only", "r.fa"], b"--keep does not go with --infix, --alignments or --scan\n"),
    (["batch", "edit", "-u", "1", "--alignments"] + AVA + ["r.fa"], b"--keep does not go with --infix, --alignments or --scan\n"),
    (["batch", "edit", "-u", "1", "--scan"] + AVA + ["--score-only", "r.fa"], b"--keep does not go with --infix, --alignments or --scan\n"),
    (["batch", "local"] + AVA + ["r.fa"], b"--keep needs one of --score-only and --paf\n"),
    (["batch", "local"] + AVA + ["--score-only", "--paf", "r.fa"], b"--keep needs one of --score-only and --paf\n"),
    (["batch", "edit"] + AVA + ["--paf", "r.fa"], b"--keep --paf does not go with edit (edit has no alignment here)\n"),
    (["batch", "overlap", "--all-vs-all", "--paf", "r.fa"], b"--paf does not go with --all-vs-all\n"),
], ids=["no-ava", "queries", "gpus", "min-score", "infix", "alignments", "scan", "no-format", "both-formats", "edit-paf", "paf-without-keep"])
def test_cli_keep_refusals(built, tmp_path, argv, why):
    """Refused with a message, the usage text and return code 1 before any GPU call (the files need not exist)"""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(why + b"Usage:"), p.stderr
    _usage_counts(p.stderr)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def reads_file(tmp_path_factory):
    """60 reads of 150-250 bases; every third read starts with the end of the read before it"""
    d = tmp_path_factory.mktemp("avahits")
    rng = random.Random(61)
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randint(150, 250))) for _ in range(60)]
    for k in range(0, 59, 3):
        ov = rng.randint(30, 140)
        reads[k + 1] = (reads[k][-ov:] + reads[k + 1])[:250]
    names = ["r%d" % k for k in range(60)]
    with open(d / "reads.fa", "w") as fh:
        for n, r in zip(names, reads):
            fh.write(">%s\n%s\n" % (n, r))
    return d, names, reads


def _run(d, argv):
    p = subprocess.run([EXE, "batch"] + argv + ["reads.fa"], cwd=d, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _values(lines, edit):
    return [int(ln.rsplit("edit_distance=", 1)[1]) if edit else int(float(ln.rsplit("score=", 1)[1])) for ln in lines]


def _two_thresholds(lines, edit):
    """the two extreme thresholds that keep at least 10 lines and drop at least 10"""
    v = _values(lines, edit)
    kept = lambda T: sum(1 for x in v if (x <= T if edit else x >= T))
    ok = [T for T in sorted(set(v)) if 10 <= kept(T) <= len(v) - 10]
    assert len(ok) >= 2
    return ok[0], ok[-1]


@pytest.mark.gpu
def test_cli_keep_score_only_overlap_is_min_score(built, reads_file):
    d, _, _ = reads_file
    dense = _run(d, ["overlap", "--all-vs-all", "--score-only"]).decode().splitlines()
    for T in _two_thresholds(dense, False):
        want = _run(d, ["overlap", "--all-vs-all", "--score-only", "--min-score", str(T)])
        assert 10 <= len(want.splitlines()) <= len(dense) - 10, T
        assert _run(d, ["overlap", "--all-vs-all", "--keep", str(T), "--score-only"]) == want, T


@pytest.mark.gpu
@pytest.mark.parametrize("cmd,opts", [("local", ["-m", "2"]), ("edit", ["-u", "1"])])
def test_cli_keep_score_only_is_the_dense_run_filtered(built, reads_file, cmd, opts):
    d, _, _ = reads_file
    edit = cmd == "edit"
    dense = _run(d, [cmd] + opts + ["--all-vs-all", "--score-only"]).decode().splitlines()
    assert len(dense) == 60 * 59 // 2
    for T in _two_thresholds(dense, edit):
        want = [ln for ln, x in zip(dense, _values(dense, edit)) if (x <= T if edit else x >= T)]
        assert 10 <= len(want) <= len(dense) - 10, (T, len(want))
        got = _run(d, [cmd] + opts + ["--all-vs-all", "--keep", str(T), "--score-only"]).decode().splitlines()
        assert got == want, T


@pytest.mark.gpu
@pytest.mark.parametrize("cmd,m", [("overlap", 1), ("local", 2), ("global", 1)])
def test_cli_keep_paf(built, reads_file, cmd, m):
    """every line's twelve columns, AS / NM and cg:Z rebuilt from Aligner.allpairs_hits(..., cigar=True)"""
    d, names, reads = reads_file
    dense = _run(d, [cmd, "-m", str(m), "--all-vs-all", "--score-only"]).decode().splitlines()
    T = _two_thresholds(dense, False)[1]
    got = _run(d, [cmd, "-m", str(m), "--all-vs-all", "--keep", str(T), "--paf"]).decode().splitlines()
    al = A.Aligner()
    al.set_scoring(m, -2, -5, -1)
    r = al.allpairs_hits(cmd, reads, T, cigar=True)
    al.close()
    assert 10 <= len(r["pair"]) <= len(dense) - 10
    want = []
    for e in range(len(r["pair"])):
        a, b, st = int(r["a"][e]), int(r["b"][e]), [int(x) for x in r["stats"][e]]
        gaps = st[4] + st[5]
        cols = [names[a], len(reads[a]), st[0], int(r["end_i"][e]), "+", names[b], len(reads[b]), st[1], int(r["end_j"][e]), st[2],
                st[2] + st[3] + gaps, 255, "AS:i:%d" % int(r["score"][e]), "NM:i:%d" % (st[3] + gaps)]
        if len(r["cigar"][e]):
            cols.append("cg:Z:" + "".join("%d%s" % (int(w) >> 4, chr(A.CIGAR_LETTERS[int(w) & 15])) for w in r["cigar"][e]))
        want.append("\t".join(str(c) for c in cols))
    assert got == want
    assert all("=" in ln.rsplit("cg:Z:", 1)[1] and "M" not in ln.rsplit("cg:Z:", 1)[1] for ln in got if "cg:Z:" in ln)
