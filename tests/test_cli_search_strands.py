"""`alignTools batch <cmd> --queries q.fa --both-strands [--best K] [--score-only] t.fa`: both strands of every query.

The refusal runs anywhere.  On the GPU the output, with the fourth column of every header line taken off, must be byte for byte
what `batch <cmd>` prints for the explicit pair file whose first records are the queries or their reverse complements -- grouped
by query, ranked (score, then target, then + before -) and cut to K -- and the column itself must be the expected strand."""
import os
import random
import subprocess

import pytest

import aligntools.c_amd as A
from conftest import ROOT

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")
SITES = " 7|30|31|60|95|140"


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("argv", [["batch", "local", "--both-strands", "t.fa"],
                                  ["batch", "fit", "-s", "--both-strands", "--score-only", "t.fa"]], ids=["local", "fit-s"])
def test_cli_both_strands_needs_queries(built, tmp_path, argv):
    """Refused with a message and return code 1 before any GPU call (the file need not exist)."""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(b"--both-strands goes with --queries") and b"--queries <queries.fa> [--best K]" in p.stderr, p.stderr
    assert b"Usage:" in p.stderr and b"[--both-strands]" in p.stderr


# ---------------------------------------------------------------- GPU
def _write(path, names, seqs, comments=None):
    with open(path, "w") as fh:
        for k, (n, s) in enumerate(zip(names, seqs)):
            fh.write(">%s%s\n" % (n, (comments or {}).get(k, "")))
            for a in range(0, len(s), 60):
                fh.write(s[a:a + 60] + "\n")


def _records(out, per):
    lines = out.decode("latin1").split("\n")[:-1]
    return ["\n".join(lines[k:k + per]) + "\n" for k in range(0, len(lines), per)]


def _value(rec):
    return float(rec.split("\n", 1)[0].split("\t")[2].split("=", 1)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("cmd,flags", [("local", []), ("fit", ["-s"])], ids=["local", "fit-s"])
def test_cli_both_strands_equals_pair_file(built, tmp_path, cmd, flags):
    rng = random.Random(len(cmd) * 11 + len(flags))
    rc = lambda s: A.revcomp(s).decode()
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    nq, nt, best = 12, 30, 3
    queries = [rnd(rng.randint(20, 140)) for _ in range(nq)]
    queries[5] = "ACGT" * 8                                                # its own reverse complement: + and - tie on every target
    targets = []
    for t in range(nt):
        if t >= 5 and rng.random() < 0.15:
            targets.append(targets[rng.randrange(t)])                      # ties
        elif rng.random() < 0.5:
            q = rng.choice(queries)
            if rng.random() < 0.5:
                q = rc(q)
            targets.append(rnd(rng.randint(0, 80)) + q + rnd(rng.randint(0, 80)))
        else:
            targets.append(rnd(rng.randint(15, 300)))
    qn = ["q%d" % k for k in range(nq)]
    tn = ["t%d" % k for k in range(nt)]
    _write(tmp_path / "q.fa", qn, queries)
    _write(tmp_path / "t.fa", tn, targets, {0: SITES} if flags else None)
    # the explicit pair file: (query, strand, target), the first record the query or its reverse complement
    pairs = [(a, s, b) for a in range(nq) for b in range(nt) for s in (0, 1) if cmd != "fit" or len(queries[a]) <= len(targets[b])]
    with open(tmp_path / "pairs.fa", "w") as fh:
        for k, (a, s, b) in enumerate(pairs):
            fh.write(">%s\n%s\n>%s%s\n%s\n" % (qn[a], rc(queries[a]) if s else queries[a], tn[b], SITES if (flags and k == 0) else "", targets[b]))
    for score_only in (False, True):
        extra = ["--score-only"] if score_only else []
        ref = subprocess.run([EXE, "batch", cmd] + flags + extra + ["pairs.fa"], cwd=tmp_path, capture_output=True, timeout=300)
        assert ref.returncode == 0, ref.stderr[-2000:]
        per = 1 if score_only else 3
        recs = _records(ref.stdout, per)
        assert len(recs) == len(pairs)
        vals = [_value(r) for r in recs]
        want, want_strand = [], []
        for a in range(nq):
            mine = [k for k, (qa, _s, _b) in enumerate(pairs) if qa == a]
            mine.sort(key=lambda k: (-vals[k], pairs[k][2], pairs[k][1]))
            want += [recs[k] for k in mine[:best]]
            want_strand += ["-" if pairs[k][1] else "+" for k in mine[:best]]
        p = subprocess.run([EXE, "batch", cmd] + flags + ["--queries", "q.fa", "--both-strands", "--best", str(best)] + extra + ["t.fa"],
                           cwd=tmp_path, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got = _records(p.stdout, per)
        assert len(got) == len(want)
        stripped, strands = [], []
        for r in got:
            head, rest = r.split("\n", 1)
            cols = head.split("\t")
            assert len(cols) == 4, head
            strands.append(cols[3])
            stripped.append("\t".join(cols[:3]) + "\n" + rest)
        assert "".join(stripped) == "".join(want), (cmd, flags, score_only)
        assert strands == want_strand, (cmd, flags, score_only)
        assert "-" in strands and "+" in strands
        assert b"[main] CMD:" in p.stderr
        # without the switch: three columns, the forward hits only
        p1 = subprocess.run([EXE, "batch", cmd] + flags + ["--queries", "q.fa", "--best", str(best)] + extra + ["t.fa"],
                            cwd=tmp_path, capture_output=True, timeout=300)
        assert p1.returncode == 0
        assert all(len(r.split("\n", 1)[0].split("\t")) == 3 for r in _records(p1.stdout, per))
