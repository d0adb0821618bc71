"""CPU: the elementwise check of oracle/norm.py on every row of the norm ledger (tests/test_hip_norm_ledger.py).  A float32
CPU evaluation - torch's own kernels with autograd, and a strictly sequential one - is scored against float64 on every
output; the worst score must stay under oracle.norm.C_NORM_REF_WORST (the kernels get four times that), and the worst of
torch's order alone under C_NORM_TORCH_WORST (the narrower bound the kernels are also held to).  The mutations a
subtly wrong kernel would leave, applied to the float32 evaluation of a row's own inputs, must each score ABOVE the kernel
tolerance on every row named for them: a row that cannot see its mutation has the wrong inputs, not the wrong tolerance."""
import pytest
import torch
import torch.nn.functional as F

from oracle import norm as N
from test_hip_norm_ledger import LEDGER, problem, row_id

# mutation -> the rows named for it
GN_FWD_MUTATIONS = {
    "one pixel dropped from one group's statistics": lambda r: r["kind"] == "gn",
    "first channel of a group normalised with the previous group's mean": lambda r: r["kind"] == "gn" and r["geom"][4] >= 2,
    # (1 / 2n of rstd: 1024 units at n = 8192 values per group, 128 at the 65536 of the 64 x 64 map)
    "divisor n - 1": lambda r: r["kind"] == "gn" and r["geom"][1] // r["geom"][4] * r["geom"][2] * r["geom"][3] <= 8192,
    # (eps / 2 var of rstd: 84 units at unit variance, 33000 at the small family's 2.5e-3)
    "eps dropped": lambda r: r["kind"] == "gn" and r["opts"]["family"] == "small",
    "FiLM scale without + 1 in one channel": lambda r: r["kind"] in ("gn", "planes", "stats") and r["opts"]["film"],
    "one-pass E[x^2] - mean^2": lambda r: r["kind"] == "gn" and r["opts"]["family"] == "offset",
    "one plane left out of the plane sum": lambda r: r["kind"] == "planes" and r["opts"]["splits"] >= 2,
}
_WORST, _WEAKEST = {}, {}


def _ragged(row):
    B, C, H, W = row["geom"]
    ppb = 256 // min(64, C // 4)
    return (B * H * W) % ppb or ppb


def _mutation_scores(row, pr):
    """{mutation: worst score over the outputs} for the mutations this row is named for"""
    out = {}
    if row["kind"] == "rms":
        m = N.rms_forward(pr.t, pr.res, mut="one pixel takes its neighbour's norm")
        out["one RMSNorm pixel takes its neighbour's norm"] = N.worst(N.scores(m, pr.ref_f, pr.S_f))
        m = N.rms_backward(pr.t, pr.mode, mut="gg without the last ragged pixel group", ragged=_ragged(row))
        out["gg summed without the last ragged pixel group"] = N.worst(N.scores(m, pr.ref_b, pr.S_b))
        return out
    for mut, named in GN_FWD_MUTATIONS.items():
        if named(row):
            out[mut] = N.worst(N.scores(pr.mutated_forward32(mut), pr.ref_f, pr.S_f))
    return out


@pytest.mark.parametrize("row", LEDGER, ids=row_id)
def test_float32_reference_passes_and_every_mutation_fails(row):
    pr = problem(row)
    tol = N.tolerance()
    rec = {}
    for sequential in (False, True):
        f, b = pr.eval32(sequential)
        sc = {f"forward {k}": v for k, v in N.scores(f, pr.ref_f, pr.S_f).items()}
        if row["kind"] != "stats":
            sc.update({f"backward {k}": v for k, v in N.scores(b, pr.ref_b, pr.S_b).items()})
        assert set(sc) >= {f"forward {k}" for k in pr.S_f if k != "xw" or row["kind"] == "planes"}
        rec["sequential" if sequential else "torch"] = sc
        at = max(sc, key=sc.get)
        print(f"[norm bounds] {row_id(row)}: float32 {'sequential' if sequential else 'torch order'}: worst {sc[at]:.2f} ({at})")
    _WORST[row_id(row)] = {k: max(v.values()) for k, v in rec.items()}
    assert max(_WORST[row_id(row)].values()) < tol
    missed = []
    for mut, score in _mutation_scores(row, pr).items():
        print(f"[norm bounds]     {mut}: {score:.3g} units (tolerance {tol:g})")
        _WEAKEST[(row_id(row), mut)] = score
        if not score > tol:
            missed.append((mut, score))
    assert missed == [], f"mutations the bound does not catch at {row_id(row)}: the row's inputs are wrong, not the bound"


def test_measured_constant_matches_the_reference():
    """C_NORM_REF_WORST in oracle/norm.py is the worst float32 reference score above, rounded up; it is never more than twice
    the measurement.  The weakest mutation is printed for the record kept next to the constant."""
    for row in LEDGER:
        if row_id(row) not in _WORST:
            test_float32_reference_passes_and_every_mutation_fails(row)
    wt = max(_WORST, key=lambda k: _WORST[k]["torch"])
    ws = max(_WORST, key=lambda k: _WORST[k]["sequential"])
    weak = min(_WEAKEST, key=_WEAKEST.get)
    worst = max(_WORST[wt]["torch"], _WORST[ws]["sequential"])
    print(f"[norm bounds] worst float32 reference: {_WORST[wt]['torch']:.2f} in torch's order at {wt}, "
          f"{_WORST[ws]['sequential']:.2f} sequential at {ws}; C_NORM_REF_WORST = {N.C_NORM_REF_WORST:g}, tolerance {N.tolerance():g}")
    print(f"[norm bounds] weakest mutation: {_WEAKEST[weak]:.1f} ({weak[1]} at {weak[0]})")
    assert worst <= N.C_NORM_REF_WORST <= 2.0 * worst
    assert _WORST[wt]["torch"] <= N.C_NORM_TORCH_WORST <= 2.0 * _WORST[wt]["torch"]
    assert N.tolerance() == 4.0 * N.C_NORM_REF_WORST and N.tolerance_blocked() == 4.0 * N.C_NORM_TORCH_WORST
    assert _WEAKEST[weak] > N.tolerance()
    assert {m for _, m in _WEAKEST} >= set(GN_FWD_MUTATIONS) | {"one RMSNorm pixel takes its neighbour's norm",
                                                               "gg summed without the last ragged pixel group"}


@pytest.mark.parametrize("film,act,res", [(True, True, True), (False, False, False)])
def test_float64_formulas_are_the_textbook_definition(film, act, res):
    """gn_forward / gn_backward (the closed form the scales are built on) against float64 autograd of F.group_norm, and the
    RMSNorm forms against F.normalize, the clamped pixel included."""
    geom = (2, 24, 3, 5, 3)
    t = N.to(N.gn_inputs(geom, "offset" if act else "plain", seed=99), torch.float64)
    ref = N.gn_autograd64(t, geom[4], film, act, res)
    f = N.gn_forward(t, geom[4], film, act, res)
    b = N.gn_backward(t, f, geom[4], film, act)
    for k in ("y",):
        assert (f[k] - ref[k]).abs().max() < 1e-11
    for k in b:
        assert (b[k] - ref[k]).abs().max() < 1e-9 * max(1.0, float(ref[k].abs().max())), k
    r = N.to(N.rms_inputs((1, 8, 3, 5), zero_pixel=True, seed=98), torch.float64)
    x, g = r["x"].clone().requires_grad_(True), r["g"].clone().requires_grad_(True)
    y = F.normalize(x, dim=1, eps=N.RMS_EPS) * g * 8 ** 0.5 + r["res"]
    y.backward(r["gy"])
    assert (N.rms_forward(r, True)["y"] - y.detach()).abs().max() < 1e-12
    assert torch.equal(N.rms_forward(r, True)["y"][1], r["res"][1])
    bb = N.rms_backward(r)
    assert (bb["gx"] - x.grad).abs().max() < 1e-9 * float(x.grad.abs().max()) and (bb["gg"] - g.grad).abs().max() < 1e-10
    assert float(x.grad[1].abs().max()) > 1e10          # below the clamp x / 1e-12 is linear: gy g sqrt(C) / 1e-12
