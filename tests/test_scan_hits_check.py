"""The selection rule of at_scan_hits (csrc/at_scanhits.h) as a stand-alone program under AddressSanitizer and UBSan:
tests/c/scanhits_check.cpp, built by `make -C aligntools/c_amd asan`.  No GPU, nothing of the library or of Python runs under a
sanitizer."""
import os

from test_asan import _run, asan          # noqa: F401  (the `make asan` fixture and the sanitizer-aware runner)


def test_scan_hits_selection_rule(asan):
    rc, out, err = _run([os.path.join(asan, "scanhits_check")])
    assert rc == 0 and "scanhits_check: ok" in out, out[-3000:] + err[-3000:]
