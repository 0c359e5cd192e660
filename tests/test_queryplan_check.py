"""The host arithmetic of the query-vs-target entries (csrc/at_queryplan.h) as a stand-alone program under AddressSanitizer and UBSan:
tests/c/queryplan_check.cpp, built by `make -C aligntools/c_amd asan`.  No GPU, nothing of the library or of Python runs under a sanitizer."""
import os

from test_asan import _run, asan          # noqa: F401  (the `make asan` fixture and the sanitizer-aware runner)


def test_query_plan_invariants(asan):
    rc, out, err = _run([os.path.join(asan, "queryplan_check")])
    assert rc == 0 and "queryplan_check: ok" in out, out[-3000:] + err[-3000:]
