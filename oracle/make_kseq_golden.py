#!/usr/bin/env python3
"""Record what the reference's own FASTA reader (klib's kseq.h from the reference's src/ directory, behind
tests/c/kseq_harness.c) makes of the hostile files of tests/test_reader.py (kseq_inputs), and write
tests/golden/kseq_records.txt: the ground truth test_both_readers_equal_the_reference_kseq holds both readers against.
The harness is compiled in a temporary directory and is not kept.  Test infrastructure.

    python oracle/make_kseq_golden.py <reference>/src
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "kseq_records.txt")


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "kseq.h")):
        sys.exit("usage: make_kseq_golden.py REFERENCE_SRC_DIR (the directory that holds the reference's kseq.h)")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reader import kseq_inputs
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "kseq_harness")
        subprocess.run(["gcc", "-std=gnu99", "-O1", "-w", "-I" + sys.argv[1], os.path.join(ROOT, "tests", "c", "kseq_harness.c"),
                        "-o", exe, "-lz"], check=True)
        files = kseq_inputs(d)
        r = subprocess.run([exe] + files, cwd=d, capture_output=True, timeout=600, check=True)
    with open(OUT, "wb") as f:
        f.write(r.stdout)
    print("%s: %d files, %d bytes" % (OUT, len(files), len(r.stdout)))


if __name__ == "__main__":
    main()
