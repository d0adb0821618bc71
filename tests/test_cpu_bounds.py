"""CPU: the elementwise forward-error check of oracle/bounds.py on every shape of the kernel ledger
(tests/test_hip_kernel_ledger.py).  A float32 CPU evaluation - torch's own order over the whole output, a strictly
sequential sum on a slice - must pass at the tolerance; five mutations a subtly wrong kernel would leave must each FAIL
it.  The ratio of norms the per-op tests use is printed next to every score: most mutations stay below its 1e-4."""
import math

import pytest
import torch

from oracle import bounds
from test_hip_kernel_ledger import KINDS, LEDGER, RTOL

PROBLEMS = sorted({(kind, r["geom"]) for r in LEDGER for kind in KINDS[r["entry"]]})
_CACHE = {}


def _problem(kind, geom):
    """one problem at a time in memory (the largest float64 outputs are 50 MB)"""
    if _CACHE.get("key") != (kind, geom):
        _CACHE.clear()
        pr = bounds.Problem(kind, geom)
        _CACHE.update(key=(kind, geom), pr=pr, got=pr.eval32())
    return _CACHE["pr"], _CACHE["got"]


def _id(p):
    return f"{p[0]}-{'x'.join(map(str, p[1]))}"


def test_forward_error_units_counts_in_units_of_the_absolute_value_sum():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    S = torch.tensor([4.0, 2.0, 0.0], dtype=torch.float64)
    assert bounds.forward_error_units(ref.float(), ref, S) == 0.0
    got = ref.clone()
    got[0] += 3 * bounds.UNIT * 4.0
    assert bounds.forward_error_units(got, ref, S) == pytest.approx(3.0)
    got = ref.clone()
    got[2] = 1e-30                                  # S == 0: exactly 0 or nothing
    assert math.isinf(bounds.forward_error_units(got, ref, S))
    got = ref.clone()
    got[1] = float("nan")
    assert math.isinf(bounds.forward_error_units(got, ref, S))
    assert bounds.tolerance(100000) == bounds.C == 4 * bounds.C_REF_WORST
    assert bounds.tolerance(3) == 12.0              # the theorem caps short reductions: 2 * (n + splits + 2), splits = 1


_WORST = {}


@pytest.mark.parametrize("prob", PROBLEMS, ids=_id)
def test_float32_reference_passes_and_every_mutation_fails(prob):
    kind, geom = prob
    pr, got = _problem(kind, geom)
    tol = bounds.tolerance(pr.n)
    own = pr.score(got)
    seq, elems = pr.eval32_sequential()
    _WORST[prob] = max(own, seq)
    print(f"[bounds] {_id(prob)}: n = {pr.n}: float32 reference {own:.2f} (torch order), {seq:.2f} (sequential, {len(elems)} "
          f"elements); tolerance {tol:g}; rel {bounds.rel(got, pr.ref):.1e}")
    assert own < tol and seq < tol
    passed = []
    for name, m in pr.mutations(got).items():
        score, r = pr.score(m), bounds.rel(m, pr.ref)
        print(f"[bounds]     {name}: {score:.3g} units, rel {r:.1e}{'  (below RTOL: the norm check misses it)' if r < RTOL else ''}")
        if not score > tol:
            passed.append((name, score))
    assert passed == [], f"mutations the bound does not catch at {_id(prob)}: the shape is wrong, not the bound"


def test_measured_constant_matches_the_reference():
    """C_REF_WORST in oracle/bounds.py is the worst score above, rounded up.  torch's own summation order depends on the
    thread count and the instruction set of the machine, so the measured value may move by a few tenths: a quarter of
    slack above the constant, and the constant never more than twice the measurement."""
    if len(_WORST) < len(PROBLEMS):
        for prob in PROBLEMS:
            if prob not in _WORST:
                pr, got = _problem(*prob)
                _WORST[prob] = max(pr.score(got), pr.eval32_sequential()[0])
    worst = max(_WORST.values())
    at = max(_WORST, key=_WORST.get)
    print(f"[bounds] worst float32 reference score {worst:.2f} at {_id(at)}; C_REF_WORST = {bounds.C_REF_WORST:g}, C = {bounds.C:g}")
    assert worst <= 1.25 * bounds.C_REF_WORST and bounds.C_REF_WORST <= 2.0 * worst
