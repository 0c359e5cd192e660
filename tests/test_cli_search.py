"""`alignTools batch <cmd> --queries q.fa [--best K] [--min-score T] [--score-only] t.fa`: every query against every target, the
best K hits per query.  The refusals run anywhere; on the GPU the output must be, byte for byte, the lines `batch <cmd>` prints
for the explicit q x t pair file, grouped by query, rank-ordered, cut to K and filtered by the cutoff."""
import os
import random
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "aligntools", "c_amd", "bin", "alignTools")


@pytest.fixture(scope="module")
def built():
    from aligntools.c_amd import build
    build.build()
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("argv,msg", [
    (["batch", "local", "--queries", "q.fa", "--all-vs-all", "t.fa"], b"--queries does not go with --all-vs-all"),
    (["batch", "overlap", "--all-vs-all", "--score-only", "--queries", "q.fa", "t.fa"], b"--queries does not go with --all-vs-all"),
    (["batch", "local", "--queries", "q.fa", "--gpus", "2", "t.fa"], b"--queries runs on one GPU"),
    (["batch", "edit", "--queries", "q.fa", "--min-score", "3", "t.fa"], b"--min-score does not go with `batch edit --queries`"),
    (["batch", "local", "--best", "3", "t.fa"], b"--best goes with --queries"),
    (["batch", "local", "--queries", "q.fa", "--best", "65", "t.fa"], b"--best K needs 1 <= K <= 64"),
    (["batch", "local", "--queries", "q.fa", "--best", "0", "t.fa"], b"--best K needs 1 <= K <= 64"),
], ids=["all-vs-all", "all-vs-all-overlap", "gpus", "edit-min-score", "best-alone", "best-65", "best-0"])
def test_cli_search_refusals(built, tmp_path, argv, msg):
    """Refused with a message and return code 1 before any GPU call (the files need not exist)."""
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(msg) and b"--queries <queries.fa> [--best K]" in p.stderr, p.stderr


def test_cli_min_score_refusal_unchanged(built, tmp_path):
    p = subprocess.run([EXE, "batch", "local", "--all-vs-all", "--score-only", "--min-score", "5", "r.fa"], cwd=tmp_path, capture_output=True)
    assert p.returncode == 1 and p.stderr.startswith(b"--min-score goes with `batch overlap --all-vs-all --score-only`\n")


# ---------------------------------------------------------------- GPU
SITES = " 7|30|31|60|95|140"


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
    head = rec.split("\n", 1)[0]
    v = head.split("\t")[2].split("=", 1)[1]
    return float(v)


@pytest.mark.gpu
@pytest.mark.parametrize("cmd,flags", [("global", []), ("local", []), ("fit", []), ("fit", ["-s"]), ("overlap", []), ("edit", [])],
                         ids=["global", "local", "fit", "fit-s", "overlap", "edit"])
def test_cli_search_equals_pair_file(built, tmp_path, cmd, flags):
    rng = random.Random(len(cmd) * 7 + len(flags))
    nq, nt = 14, 40
    queries = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 160))) for _ in range(nq)]
    targets = []
    for t in range(nt):
        if t >= 5 and rng.random() < 0.15:
            targets.append(targets[rng.randrange(t)])                      # ties
        elif rng.random() < 0.4:
            q = rng.choice(queries)
            targets.append("".join(rng.choice("ACGT") for _ in range(rng.randint(0, 80))) + q + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 80))))
        else:
            targets.append("".join(rng.choice("ACGT") for _ in range(rng.randint(15, 300))))
    qn = ["q%d" % k for k in range(nq)]
    tn = ["t%d" % k for k in range(nt)]
    _write(tmp_path / "q.fa", qn, queries)
    _write(tmp_path / "t.fa", tn, targets, {0: SITES} if flags else None)
    # the explicit pair file: every (query, target), query-major (fit: only pairs with the query no longer than the target)
    pairs = [(a, b) for a in range(nq) for b in range(nt) if cmd != "fit" or len(queries[a]) <= len(targets[b])]
    with open(tmp_path / "pairs.fa", "w") as fh:
        for k, (a, b) in enumerate(pairs):
            fh.write(">%s\n%s\n>%s%s\n%s\n" % (qn[a], queries[a], tn[b], SITES if (flags and k == 0) else "", targets[b]))
    for score_only in ([False, True] if cmd != "edit" else [False]):
        extra = ["--score-only"] if score_only else []
        ref = subprocess.run([EXE, "batch", cmd] + flags + extra + ["pairs.fa"], cwd=tmp_path, capture_output=True, timeout=300)
        assert ref.returncode == 0, ref.stderr[-2000:]
        per = 1 if (score_only or cmd == "edit") else 3
        recs = _records(ref.stdout, per)
        assert len(recs) == len(pairs)
        vals = [_value(r) for r in recs]
        cut_at = sorted(vals)[len(vals) // 2]
        for best in (1, 5):
            for cutoff in ([None, int(cut_at)] if cmd != "edit" else [None]):
                want = []
                for a in range(nq):
                    mine = [(k, b) for k, (qa, b) in enumerate(pairs) if qa == a]
                    if cutoff is not None:
                        mine = [(k, b) for k, b in mine if vals[k] >= cutoff]
                    sign = 1 if cmd == "edit" else -1
                    mine.sort(key=lambda kb: (sign * vals[kb[0]], kb[1]))
                    want += [recs[k] for k, _ in mine[:best]]
                argv = [EXE, "batch", cmd] + flags + ["--queries", "q.fa", "--best", str(best)] + extra
                if cutoff is not None:
                    argv += ["--min-score", str(cutoff)]
                p = subprocess.run(argv + ["t.fa"], cwd=tmp_path, capture_output=True, timeout=300)
                assert p.returncode == 0, p.stderr[-2000:]
                assert p.stdout.decode("latin1") == "".join(want), (cmd, flags, score_only, best, cutoff)
                assert b"[main] CMD:" in p.stderr
