"""CPU: the forward-error check of oracle/streaming.py on every case of tests/test_hip_streaming.py.  The float32 CPU
evaluation of each operation must pass at the tolerance; every deviation a subtly wrong kernel would leave must FAIL it.
The tolerances are measured here: C_REF_WORST_<family> is the worst float32 score of the family, the tolerance 4 times that.
Every score and every mutation's score is printed (pytest -s / -rP).  Nothing here runs a HIP kernel."""
import math

import pytest
import torch

from oracle import streaming as st

_CASES = {}
_WORST = {}


def _cases(family):
    if family not in _CASES:
        _CASES[family] = st.FAMILIES[family]()
    return _CASES[family]


def _evaluations(case):
    """{label: float32 result}: the plain formula, and torch's own implementation / another order where there is one"""
    out = {"float32 formula": case.eval32()}
    if hasattr(case, "eval32_torch"):
        out["torch.optim, float32, foreach=False"] = case.eval32_torch()
    if hasattr(case, "eval32_sequential"):
        out["strictly sequential float32 sum"] = case.eval32_sequential()
    return out


def _run_family(family):
    worst, failures = (0.0, None), []
    for case in _cases(family):
        evals = _evaluations(case)
        for label, got in evals.items():
            sc = case.scores(got)
            print(f"[streaming] {case.name}: {label}: " + ", ".join(f"{k} {v:.2f}" for k, v in sc.items()) + f"; tolerance {case.tol:g}")
            top = max(sc.values())
            if top > worst[0]:
                worst = (top, f"{case.name} ({label}: {max(sc, key=sc.get)})")
            if not top < case.tol:
                failures.append((case.name, label, sc))
        got = evals["float32 formula"]
        for name, m in case.mutations(got).items():
            s = case.score(m)
            print(f"[streaming]     mutation: {name}: {s:.3g} units")
            if not s > case.tol:
                failures.append((case.name, "mutation passes: " + name, s))
        for name, m in case.reported(got).items():
            print(f"[streaming]     reported: {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in case.scores(m).items()))
    _WORST[family] = worst
    return failures


@pytest.mark.parametrize("family", sorted(st.FAMILIES))
def test_float32_reference_passes_and_every_mutation_fails(family):
    failures = _run_family(family)
    assert failures == [], f"{family}: if a shape lets a mutation pass, the shape is wrong, not the bound"


@pytest.mark.parametrize("family", sorted(st.FAMILIES))
def test_measured_constant_matches_the_reference(family):
    """C_REF_WORST_<family> in oracle/streaming.py is the worst float32 score above, rounded up: a quarter of slack above the
    constant (torch's vectorised order and libm move the measurement by tenths between machines), and the constant never
    more than twice the measurement."""
    if family not in _WORST:
        _run_family(family)
    worst, at = _WORST[family]
    C = st.C_REF_WORST[family]
    print(f"[streaming] {family}: worst float32 reference score {worst:.2f} at {at}; C_REF_WORST = {C:g}, tolerance {4 * C:g}")
    assert worst <= 1.25 * C and C <= 2.0 * worst


@pytest.mark.parametrize("config", sorted(st.ADAM_CONFIGS))
def test_adam_formula_is_torch_optim(config):
    """adam_formula in float64 IS torch.optim.Adam / AdamW in float64: five chained steps to 1e-12, so the reference of every
    Adam check is torch's and not ours."""
    hp = st.ADAM_CONFIGS[config]
    p, _, m, v = (t.double() for t in st.adam_inputs(515, 1))
    par = p.clone().requires_grad_(True)
    cls = torch.optim.AdamW if hp["decoupled"] else torch.optim.Adam
    opt = cls([par], lr=hp["lr"], betas=hp["betas"], eps=st.ADAM_EPS, weight_decay=hp["wd"], foreach=False)
    for step in range(1, 6):
        g = st.adam_inputs(515, 1, seed=step)[1].double()
        par.grad = g * hp["grad_scale"]
        opt.step()
        ours, _ = st.adam_formula(p, g, m, v, step, **hp)
        p, m, v = ours["p"], ours["m"], ours["v"]
        for got, want in ((p, par.detach()), (m, opt.state[par]["exp_avg"]), (v, opt.state[par]["exp_avg_sq"])):
            assert float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) < 1e-12
    # and one step from an arbitrary state, the form every case uses
    ins = st.adam_inputs(515, 1000)
    ours, _ = st.adam_formula(*ins, 1000, **hp)
    theirs = st.adam_torch(*ins, 1000, **hp)
    for k in ours:
        assert float(((ours[k] - theirs[k]).abs() / theirs[k].abs().clamp_min(1e-300)).max()) < 1e-12


@pytest.mark.parametrize("config", sorted(st.RMSPROP_CONFIGS))
def test_rmsprop_formula_is_torch_optim(config):
    hp = st.RMSPROP_CONFIGS[config]
    p, g, _, v = st.adam_inputs(515, 5)
    ours, _ = st.rmsprop_formula(p, g, v, **hp)
    theirs = st.rmsprop_torch(p, g, v, **hp)
    for k in ours:
        assert float(((ours[k] - theirs[k]).abs() / theirs[k].abs().clamp_min(1e-300)).max()) < 1e-12


def test_naive_adam_companion_would_fail_the_reference():
    """|p| + |delta| as the companion of p scores torch's own float32 Adam in the hundreds: m and g + wd p cancel, and the
    companion has to carry that (oracle/streaming.py: S_p)."""
    case = st.AdamCase(3074, "coupled", 7)
    got = case.eval32_torch()
    delta = (case.ref["p"] - case.inputs[0].double()).abs()
    naive = st.forward_error_units(got["p"], case.ref["p"], case.inputs[0].double().abs() + delta)
    print(f"[streaming] naive companion: {naive:.1f} units; S_p: {case.scores(got)['p']:.2f}")
    assert naive > case.tol > case.scores(got)["p"]


def test_ema_copy_formula_is_not_a_copy():
    """s + (o - s) * 1 in float32 differs from o in most elements; torch.lerp(s, o, 1) and the oracle's "copy" do not"""
    sh, on = st.ema_inputs(3074)
    lerped = sh + (on - sh) * 1.0
    frac = float((lerped != on).float().mean())
    print(f"[streaming] s + (o - s) * 1 != o in {100 * frac:.0f} % of the elements")
    assert frac > 0.2
    assert st.exact_units(torch.lerp(sh, on, 1.0).abs(), on.abs()) == 0.0        # up to the sign of zero
    assert st.exact_units(on.clone(), on) == 0.0 and math.isinf(st.exact_units(-on, on))


def test_data_movement_references():
    g = torch.Generator().manual_seed(0)
    hi = torch.randn(2, 6, 10, 3, generator=g)
    lo = st.pixel_unshuffle(hi)
    assert lo.shape == (2, 3, 5, 12) and torch.equal(st.pixel_shuffle(lo), hi)
    assert float(lo[1, 2, 4, 2 * 4 + 1 * 2 + 0]) == float(hi[1, 5, 8, 2])          # y[b,h,w,c*4+p1*2+p2] = x[b,2h+p1,2w+p2,c]
    x = torch.randn(2, 3, 5, 4, generator=g)
    up = st.upsample2x_fwd(x)
    assert up.shape == (2, 6, 10, 4) and torch.equal(up[:, 1::2, 0::2], x) and torch.equal(up[:, 0::2, 1::2], x)
    src = torch.randn(2, 3, 3, 5, generator=g)
    nhwc = st.nchw_to_nhwc(src, 4)
    assert torch.equal(nhwc[..., :3], src.permute(0, 2, 3, 1).reshape(2, 15, 3)) and float(nhwc[..., 3].abs().max()) == 0.0
