"""CPU: the elementwise check of oracle/attention.py on every row of the attention ledger (tests/test_hip_attention_ledger.py).
Three float32 CPU evaluations - torch's own order, and online softmax over key tiles of 64 and of 128 with sequential sums - are
scored against float64 on every output; the worst score must stay under the family's constant (C_LINATTN_REF_WORST /
C_ATTN_REF_WORST; the kernels get four times that).  The mutations a subtly wrong kernel would leave, applied to the float32
evaluation of a row's own inputs, must each score ABOVE the kernel tolerance on every row named for them: a row that cannot
see its mutation has the wrong inputs, not the wrong tolerance."""
import pytest
import torch

from oracle import attention as A
from test_hip_attention_ledger import LEDGER, problem, row_id


def _la(r):
    return r["kind"] != "attn"


def _core(r):
    """(B, heads, n, M) of the attention core of a row (the fused tails have heads = 4 and M = 4)"""
    g = r["geom"]
    return (g[0], g[1], g[2] * g[3], g[4]) if r["kind"] in ("linattn", "attn") else (g[0], 4, g[2] * g[3], 4)


def _fwd(r):
    """the row checks outputs of the forward pass (the fused backward tail takes its saved values from the unfused forward)"""
    return r["kind"] != "la_bwd_tail"


def _bwd(r):
    return r["kind"] != "la_fwd_tail"


def _nk(r):
    return _core(r)[2] + _core(r)[3]


def _moves_late(r):
    """the running maximum moves in the LAST tile: a ramp, a last key that is the maximum, and for LinearAttention (memory
    columns last) a memory column that is.  In full attention the memory rows come first: "memmax" never moves it again."""
    tiles = -(-_nk(r) // (A.LA_TILE if _la(r) else A.FA_TILE))
    return _fwd(r) and tiles > 1 and (r["family"] in ("ascending", "late") or (_la(r) and r["family"] == "memmax"))


def _spike(r):
    """"spike": the last pixel's key is 20 above every other key, whose weights (e^-20 = 2e-9) are below 2^-24 of every sum:
    nothing done to a memory column or row can be seen there, only what touches the spike itself; and gq is a pure
    cancellation (LinearAttention: one channel of q carries softmax_d(q); full attention: delta_i is the spike's dp)."""
    return r["family"] == "spike"


# mutation -> the rows named for it
MUTATIONS = {
    A.M_ACC: _moves_late,
    A.M_WSUM: _moves_late,
    A.M_KSUM_MEM: lambda r: _la(r) and _fwd(r) and _core(r)[3] > 0 and not _spike(r),
    # LinearAttention: the last pixel of a tile that is not full; full attention: the last key of a ragged key tile
    A.M_DROP: lambda r: _fwd(r) and ((_core(r)[2] % A.LA_TILE != 0) if _la(r) else (_nk(r) % A.FA_TILE != 0 and _core(r)[2] > 1)),
    A.M_STRIDE: lambda r: _fwd(r) and _core(r)[3] >= 2 and not _spike(r),
    # (a single key: gq is pure cancellation, 0 with or without the factor.  LinearAttention "memmax": every column d of k puts
    # its whole weight on memory column 0, all rows of ctx are that column's v, and g1 - dot cancels in the same way)
    A.M_SCALE2: lambda r: _bwd(r) and not _spike(r) and (r["family"] != "memmax" if _la(r) else _nk(r) > 1),
    A.M_LSE: lambda r: not _la(r),
    # (visible where the denominator is not 1: not where one key carries the whole row)
    A.M_DELTA: lambda r: not _la(r) and r["family"] in ("plain", "ascending", "peaked") and _nk(r) > 1,
    A.M_HEAD: lambda r: _fwd(r) and _core(r)[0] >= 2 and _core(r)[1] >= 2 and _core(r)[3] > 0 and not _spike(r),
    A.M_RVEC: lambda r: _la(r) and _bwd(r),
}
_WORST, _WEAKEST = {}, {}


def _fam_const(kind):
    return A.C_ATTN_REF_WORST if kind == "attn" else A.C_LINATTN_REF_WORST


@pytest.mark.parametrize("row", LEDGER, ids=row_id)
def test_float32_reference_passes_and_every_mutation_fails(row):
    pr = problem(row)
    tol = A.tolerance(row["kind"])
    assert tol == 4.0 * _fam_const(row["kind"])
    worst = {}
    for order in A.ORDERS:
        sc = A.scores(pr.eval32(order), pr.ref, pr.S)
        assert set(sc) == set(pr.S)
        at = max(sc, key=sc.get)
        worst[order] = (sc[at], at)
        print(f"[attention bounds] {row_id(row)}: float32 {order}: worst {sc[at]:.2f} ({at})")
    _WORST[row_id(row)] = ("attn" if row["kind"] == "attn" else "linattn", max(v[0] for v in worst.values()))
    assert _WORST[row_id(row)][1] < _fam_const(row["kind"])
    missed = []
    for mut, named in MUTATIONS.items():
        if not named(row):
            continue
        score = A.worst(A.scores(pr.mutated32(mut), pr.ref, pr.S))
        print(f"[attention bounds]     {mut}: {score:.3g} units (tolerance {tol:g})")
        _WEAKEST[(row_id(row), mut)] = score
        if not score > tol:
            missed.append((mut, score))
    assert missed == [], f"mutations the bound does not catch at {row_id(row)}: the row's inputs are wrong, not the bound"


def test_measured_constants_match_the_reference():
    """C_LINATTN_REF_WORST and C_ATTN_REF_WORST in oracle/attention.py are the worst float32 reference scores above, rounded
    up, never more than twice the measurement; tolerance() is four times them; the weakest mutation is above the tolerance."""
    for row in LEDGER:
        if row_id(row) not in _WORST:
            test_float32_reference_passes_and_every_mutation_fails(row)
    for kind in ("linattn", "attn"):
        rows = {k: v[1] for k, v in _WORST.items() if v[0] == kind}
        at = max(rows, key=rows.get)
        c = _fam_const(kind)
        print(f"[attention bounds] worst float32 reference of {kind}: {rows[at]:.2f} at {at}; constant {c:g}, tolerance {A.tolerance(kind):g}")
        assert rows[at] <= c <= 2.0 * rows[at]
        assert A.tolerance(kind) == 4.0 * c
        weak = min((k for k in _WEAKEST if k[0] in rows), key=_WEAKEST.get)
        print(f"[attention bounds] weakest mutation of {kind}: {_WEAKEST[weak]:.1f} ({weak[1]} at {weak[0]})")
        assert _WEAKEST[weak] > A.tolerance(kind)
    assert {m for _, m in _WEAKEST} == set(MUTATIONS)
    # every mutation is seen by at least one row of each family it applies to
    for kind in ("linattn", "attn"):
        seen = {m for (rid, m) in _WEAKEST if _WORST[rid][0] == kind}
        assert seen == set(MUTATIONS) - ({A.M_LSE, A.M_DELTA} if kind == "linattn" else {A.M_KSUM_MEM, A.M_RVEC})


@pytest.mark.parametrize("family", ["plain", "ascending"])
def test_float64_formulas_are_the_textbook_definition(family):
    """la_forward / la_backward and fa_forward / fa_backward (the closed forms the scales are built on) against float64
    autograd of the reference's own formulation, at a tiny shape with two images, three heads and three memory columns."""
    geom = (2, 3, 2, 3, 3)
    for kind, auto in (("linattn", A.la_autograd64), ("attn", A.fa_autograd64)):
        pr = A.Problem(kind, geom, family, seed=97)
        want = auto(pr.t)
        for k, w in want.items():
            assert (pr.ref[k] - w).abs().max() < 1e-12 * max(1.0, float(w.abs().max())), (kind, k)
        assert all(bool((pr.S[k] >= pr.ref[k].abs() * (1 - 1e-12)).all()) for k in pr.S)     # a scale is never below its value
    # kmax is the exact column maximum over memory columns and pixels
    pr = A.Problem("linattn", geom, "memmax", seed=96)
    kk = torch.cat((pr.t["k"], pr.t["mem"][0].expand(2, -1, -1, -1)), -1)
    assert torch.equal(pr.ref["kmax"].float(), kk.max(-1).values)
    assert float(pr.ref["kmax"].min()) > 10.0            # the memory column at 16 carries it
