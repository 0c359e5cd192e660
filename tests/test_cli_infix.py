"""`alignTools batch edit -u 1 --infix`: the distance of the best match of the first sequence inside the second (at_set_edit_infix), on
pair files and on --queries; with --alignments --paf the target start and end columns of the PAF line are where the match lies.

The refusals run anywhere.  On the GPU the expected output is built from the Python API (Aligner.set_edit_infix, align_batch, search,
the host CIGAR) and compared byte for byte with the binary's."""
import os
import random
import subprocess

import pytest

import aligntools.c_amd as A
from conftest import ROOT

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("argv,why", [
    (["batch", "local", "--infix", "p.fa"], b"--infix goes with edit\n"),
    (["batch", "edit", "--infix", "p.fa"], b"--infix needs -u 1\n"),
    (["batch", "edit", "-u", "2", "--infix", "--queries", "q.fa", "t.fa"], b"--infix needs -u 1\n"),
    (["batch", "edit", "-u", "1", "--all-vs-all", "--infix", "p.fa"], b"--infix does not go with --all-vs-all\n"),
    (["batch", "edit", "-u", "1", "--gpus", "2", "--infix", "p.fa"], b"--infix runs on one GPU: it does not go with --gpus N > 1\n"),
], ids=["not-edit", "default-u", "u-2", "all-vs-all", "gpus"])
def test_cli_infix_refusals(built, tmp_path, argv, why):
    """Refused with a message, the usage line and return code 1 before any GPU call (the files need not exist)"""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(why + b"Usage:"), p.stderr
    assert p.stderr.count(b"[--infix]") == 2


def test_cli_usage_text_keeps_its_shape(built, tmp_path):
    p = subprocess.run([EXE, "batch", "edit", "-u", "1", "--gpus", "2", "--infix", "p.fa"], cwd=tmp_path, capture_output=True, timeout=60)
    assert p.stderr.count(b"[--paf]") == 2 and p.stderr.count(b"[--alignments]") == 2 and p.stderr.count(b"[--infix]") == 2
    lines = [ln for ln in p.stderr.split(b"\n") if b"alignTools batch" in ln]
    assert len(lines) == 2 and b"<pairs.fa>" in lines[0] and b"<targets.fa>" in lines[1]
    assert b"--queries <queries.fa> [--best K] [--both-strands]" in lines[1]
    assert b"--queries <queries.fa> [--best K] [--both-strands]" in p.stderr


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def al():
    a = A.Aligner()
    a.set_scoring(1, 1, -5, -1, -10)
    a.set_edit_traceback(True)
    a.set_edit_infix(True)
    yield a
    a.close()


def _expected(al, items):
    """items: (qname, query as in the file, strand, tname, target) -> (PAF lines, plain records)"""
    pairs = [(A.revcomp(q) if s == "-" else q.encode(), t.encode()) for _qn, q, s, _tn, t in items]
    r = al.align_batch("edit", pairs)
    assert al.last_config.startswith("myers-infix-tb"), al.last_config
    paf, plain = [], []
    for k, (qn, q, s, tn, t) in enumerate(items):
        end_i, end_j, dist = int(r["end_i"][k]), int(r["end_j"][k]), int(r["score"][k])
        words, st = A.cigar(r["ops"][k], pairs[k][0], end_i, pairs[k][1], end_j)
        st = [int(x) for x in st]
        assert st[3] + st[4] + st[5] == dist and end_i == len(q) and st[0] == 0
        qs, qe = (st[0], end_i) if s == "+" else (len(q) - end_i, len(q) - st[0])
        cols = [qn, len(q), qs, qe, s, tn, len(t), st[1], end_j, st[2], st[2] + st[3] + st[4] + st[5], 255]
        line = "\t".join(str(c) for c in cols) + "\tAS:i:%d\tNM:i:%d" % (-dist, dist)
        if len(words):
            line += "\tcg:Z:" + A.cigar_string(words).decode()
        paf.append(line + "\n")
        plain.append((qn, tn, "edit_distance=%d" % dist, r["r1"][k], r["r2"][k]))
    return paf, plain


@pytest.mark.gpu
def test_cli_infix_pair_file(built, al, tmp_path):
    rng = random.Random(31)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    items = []
    for k in range(11):
        a = rnd(rng.randint(1, 70))
        inside = a[:len(a) // 2] + rnd(k % 3) + a[len(a) // 2 + k % 2:]
        b = (rnd(rng.randint(0, 90)) + inside + rnd(rng.randint(0, 60))) if k % 4 else rnd(rng.randint(1, 80))
        items.append(("a%d" % k, a, "+", "b%d" % k, b))
    items.append(("read", "ACGT", "+", "repeat", "ACGTACGTACGT"))
    items.append(("long", "ACGTA", "+", "short", "CG"))
    with open(tmp_path / "p.fa", "w") as fh:
        for qn, q, _s, tn, t in items:
            fh.write(">%s\n%s\n>%s\n%s\n" % (qn, q, tn, t))
    paf, plain = _expected(al, items)
    assert paf[11].split("\t")[7:9] == ["0", "4"] and any(int(x.split("\t")[7]) > 0 for x in paf)
    p = subprocess.run([EXE, "batch", "edit", "-u", "1", "--infix", "--alignments", "--paf", "p.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf
    p = subprocess.run([EXE, "batch", "edit", "-u", "1", "--alignments", "--infix", "p.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("%s\t%s\t%s\n%s\n%s\n" % rec for rec in plain)
    # without --alignments: the name lines, with the infix numbers
    p = subprocess.run([EXE, "batch", "edit", "-u", "1", "--infix", "p.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("%s\t%s\t%s\n" % rec[:3] for rec in plain)


@pytest.mark.gpu
def test_cli_infix_search_both_strands(built, al, tmp_path):
    rng = random.Random(32)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    queries = [rnd(rng.randint(20, 40)) for _ in range(6)]
    queries[2] = "ACGT" * 6                                             # its own reverse complement: + and - tie on every target
    targets = []
    for t in range(5):
        q = queries[(2 * t) % 6]
        if t % 2:
            q = A.revcomp(q).decode()
        targets.append(rnd(10 * t + 3) + q[:9] + rnd(1) + q[10:15] + q[17:] + rnd(40 - 7 * t))     # the read inside, with edits
    qn = ["q%d" % k for k in range(6)]
    tn = ["t%d" % k for k in range(5)]
    for name, names, seqs in (("q.fa", qn, queries), ("t.fa", tn, targets)):
        with open(tmp_path / name, "w") as fh:
            for n, s in zip(names, seqs):
                fh.write(">%s\n%s\n" % (n, s))
    hits = al.search("edit", queries, targets, k=2, strands="both")
    items = []
    for q in range(6):
        for j in range(int(hits["nhits"][q])):
            t = int(hits["target"][q, j])
            items.append((qn[q], queries[q], "-" if hits["strand"][q, j] == 1 else "+", tn[t], targets[t]))
    assert len(items) == 12 and {"+", "-"} == {it[2] for it in items}
    paf, plain = _expected(al, items)
    argv = [EXE, "batch", "edit", "-u", "1", "--infix", "--queries", "q.fa", "--best", "2", "--both-strands", "--alignments"]
    p = subprocess.run(argv + ["--paf", "t.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode().splitlines(keepends=True) == paf
    p = subprocess.run(argv + ["t.fa"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("%s\t%s\t%s\t%s\n%s\n%s\n" % (a, b, sc, it[2], r1, r2) for (a, b, sc, r1, r2), it in zip(plain, items))
