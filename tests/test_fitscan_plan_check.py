"""The fit scan's planner (csrc/at_fitscan_plan.h) as a stand-alone program under AddressSanitizer and UBSan:
tests/c/fitscan_plan_check.cpp, built by `make -C aligntools/c_amd asan`.  No GPU, nothing of the library or of Python runs under a
sanitizer."""
import os

from test_asan import _run, asan          # noqa: F401  (the `make asan` fixture and the sanitizer-aware runner)


def test_fit_scan_planner_invariants(asan):
    rc, out, err = _run([os.path.join(asan, "fitscan_plan_check")])
    assert rc == 0 and "fitscan_plan_check: ok" in out, out[-3000:] + err[-3000:]
