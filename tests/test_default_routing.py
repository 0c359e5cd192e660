"""GPU suite: the routing users get.  tests/test_gpu_parity.py runs under AT_PACKED_MIN_ROUNDS=0 so that its small batches reach the
64-lane packed kernels; here nothing is set: small batches take whatever kernel align_device picks for them by default (mostly the
int32 kernel, the packed ones from one round of the resident waves up), and the results are the reference's all the same."""
import os
import random

import pytest

import oracle as O   # test infrastructure: the checker
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al():
    import aligntools.c_amd as A
    saved = {k: os.environ.pop(k) for k in ("AT_PACKED_MIN_ROUNDS", "AT_NO_PACKED", "AT_GROUP", "AT_TAIL_SPLIT") if k in os.environ}
    a = A.Aligner()
    yield a
    a.close()
    os.environ.update(saved)


def test_goldens_under_default_routing(al):
    from test_gpu_parity import _group, _run_group
    seen = set()
    for name in ("random_small.jsonl", "random_dna.jsonl", "known_answers.jsonl"):
        for key, cases in _group(load_golden(name)).items():
            _run_group(al, key, cases)
            seen.add(al.last_config.split(" store=")[0])
    assert any(c.startswith("int32") for c in seen) and any(c.startswith("packed16") for c in seen), seen


def test_batches_on_both_sides_of_the_packed_threshold(al):
    """Uniform global batches of 1024 x 1024 (64-lane packed kernel, two alignments per wave): 600 pairs are less than one round of the
    resident waves and stay on the int32 kernel, 7 000 take the packed one -- the same answers from both (sample against the oracle)."""
    rng = random.Random(77)
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    base = [(dna(1024), dna(1024)) for _ in range(40)]
    al.set_scoring(1, -1, -4, -1)
    small = al.align_batch("global", base * 15, render=False)
    assert "int32" in al.last_config, al.last_config
    big = al.align_batch("global", base * 175, render=False)
    assert "packed16 x4" in al.last_config and "1x64-lane" in al.last_config, al.last_config
    for k in range(40):
        r = O.align(O.GLOBAL, base[k][0], base[k][1], 1, -1, -4, -1)
        for res, q in ((small, k), (small, 40 * 14 + k), (big, k), (big, 40 * 174 + k)):
            assert (int(res["score"][q]), int(res["state"][q]), res["ops"][q]) == (r["score"], r["state"], r["ops"]), (k, q)


def test_small_ragged_overlap_batch_with_tracebacks_stays_on_the_packed_kernel(al):
    """A ragged overlap batch with tracebacks is planned for the packed overlap kernel's frames: runs of equal l1 padded to whole work
    items with ~index repeats.  Such a launch must not fall back to the int32 kernel for being small (the rule that keeps small uniform
    64-lane batches there), which reads the order's entries as they are.  A few hundred pairs of short reads against short second
    sequences, read lengths that occur once or an odd number of times, both row classes, both alphabets: packed frames under the
    default routing, every result the oracle's."""
    rng = random.Random(6464)
    for alpha in ("ACGT", "ACGTN"):
        dna = lambda n: "".join(rng.choice(alpha) for _ in range(n))
        pairs = []
        for k in range(301):
            l1 = rng.choice([1, 2, 17, 60, 255, 256, 257, 304]) if k % 3 else rng.randint(1, 304)
            l2 = max(1, l1 - 40 + rng.choice([0, 2, 30, 150]))
            a = dna(l1)
            if k % 4:
                ov = rng.randint(1, min(l1, l2))
                b = (a[l1 - ov:] + dna(l2))[:l2]
            else:
                b = dna(l2)
            pairs.append((a, b))
        for sc in ((1, -1, -2, -1), (1, -2, -5, -1)):
            al.set_scoring(*sc)
            res = al.align_batch("overlap", pairs, render=False)
            assert "packed16 x4" in al.last_config and "ragged frames" in al.last_config, al.last_config
            for k, (a, b) in enumerate(pairs):
                r = O.align(O.OVERLAP, a, b, *sc)
                assert (int(res["score"][k]), int(res["end_i"][k]), int(res["end_j"][k]), res["ops"][k]) == \
                       (r["score"], r["end_i"], r["end_j"], r["ops"]), (alpha, sc, k, len(a), len(b))
