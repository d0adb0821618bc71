"""CPU: the gradient tail - global-norm clipping and gradient accumulation - without a GPU.

The float32 evaluation of a clipped Adam step is measured against the float64 reference of tests/gradtail_ref.py (this fixes
the tolerance the GPU tests use), every mutation of the clip scale must fail that tolerance on the cases the reference names,
MiniTrainer clips a CPU plumbing model exactly as a hand-written loop with torch.nn.utils.clip_grad_norm_ does, and the
host-only queries of the new entry points answer without a device."""
import copy
import math

import pytest
import torch
from torch import nn

import gradtail_ref as gr
from oracle import streaming as st


# ---- the reference and its float32 evaluation -----------------------------------------------------------------------------------

def test_float32_evaluation_of_the_clipped_update_stays_within_the_adam_constant():
    """float32 norm, scale rounded once to float32, torch's Adam formula in float32 - against adam_formula in float64 with
    grad_scale * coef from the float64 norm.  Measured: 6.17 units (v, clip-coupled-n3074-step1000, every max_norm), so
    C_REF_WORST_ADAM = 6.5 and the tolerance of 26 units hold unchanged."""
    worst, where = 0.0, None
    for case in gr.clip_cases():
        for k, u in case.scores(case.eval32()).items():
            if u > worst:
                worst, where = u, f"{case.name}: {k}"
    print(f"[gradtail] worst float32 evaluation: {worst:.3f} units at {where}")
    assert worst <= gr.C_REF_WORST_GRADTAIL == st.C_REF_WORST_ADAM, (worst, where)
    assert gr.tolerance() == st.tolerance("adam") == 26.0


def test_the_clip_acts_in_the_cases_that_claim_it():
    """max_norm 1e-3 and 1 clip every case, 1e6 none: the reference itself separates the two regimes"""
    for case in gr.clip_cases():
        gs = case.hp["grad_scale"]
        if case.max_norm == 1e6:
            assert case.scale == gs, case.name
        elif case.max_norm == 1e-3:
            assert abs(case.scale) < abs(gs) and case.norm > case.max_norm, case.name
        assert math.isclose(case.norm, gr.norm64(case.inputs[1], gs), rel_tol=0, abs_tol=0)


@pytest.mark.parametrize("name", gr.MUTATIONS)
def test_every_mutation_of_the_scale_fails_the_tolerance(name):
    """each deviation scores far above the tolerance on at least one of the cases named for it (measured: above 1e7)"""
    scores = {c.name: c.score(c.mutation(name)) for c in gr.mutation_cases(name)}
    worst = max(scores.values())
    print(f"[gradtail] mutation {name!r}: worst {worst:.3e} units; fails on {sum(s >= gr.tolerance() for s in scores.values())}"
          f" of {len(scores)} cases")
    assert worst > 1e7, (name, scores)
    # and the unmutated float32 evaluation passes on every one of those cases
    for c in gr.mutation_cases(name):
        assert c.score(c.eval32()) < gr.tolerance(), c.name


def test_the_tiny_case_sits_where_the_1e_6_shows():
    for c in gr.mutation_cases("+ 1e-6 left out"):
        if c.n >= 1027:                                       # (five elements carry less)
            assert 1.0e-6 <= c.norm <= 2.2e-6, (c.name, c.norm)


def test_nan_and_inf_gradients():
    g = st.adam_inputs(1027, 7)[1]
    bad = g.clone()
    bad[5] = float("nan")
    scale, norm = gr.clip_scale64(bad, 0.5, 1.0)
    assert math.isnan(scale) and math.isnan(norm)             # torch's clamp propagates NaN (fminf(1, NaN) would not)
    bad[5] = float("inf")
    scale, norm = gr.clip_scale64(bad, 0.5, 1.0)
    assert scale == 0.0 and math.isinf(norm)
    scale, norm = gr.clip_scale64(torch.zeros(9), 0.125, 1.0)
    assert scale == 0.125 and norm == 0.0
    # torch itself, on the same inputs
    p = nn.Parameter(torch.zeros(1027))
    p.grad = (g * 0.5).clone()
    p.grad[5] = float("nan")
    torch.nn.utils.clip_grad_norm_([p], 1.0)
    assert bool(torch.isnan(p.grad).all())


def test_accumulate_sum_is_the_sequential_float32_sum():
    g = torch.Generator().manual_seed(3)
    gs = [torch.randn(1000, generator=g) * 10.0 ** (3 * i) for i in range(3)]
    want = (gs[0] + gs[1]) + gs[2]
    assert torch.equal(gr.accumulate_sum(gs), want)
    assert not torch.equal(want, gs[0] + (gs[1] + gs[2]))     # the order is part of the contract


# ---- MiniTrainer on a CPU plumbing model ----------------------------------------------------------------------------------------

def _net_class():
    from lgm_hip.lightning import MiniLightningModule

    class Net(MiniLightningModule):
        def __init__(self):
            super().__init__()
            self.a, self.b = nn.Linear(6, 5), nn.Linear(5, 3)

        def training_step(self, batch, batch_idx):
            x, y = batch
            loss = (self.b(torch.tanh(self.a(x))) - y).square().mean() * 50.0
            self.log("train_loss", loss.detach())
            return loss

        def configure_optimizers(self):
            return torch.optim.Adam(self.parameters(), lr=1e-2)
    return Net


def _data(n):
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(8, 6, generator=g), torch.randn(8, 3, generator=g)) for _ in range(n)]


def _params(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()])


def test_minitrainer_clips_like_a_hand_written_loop():
    """fails on a trainer that swallows ``gradient_clip_val``"""
    from lgm_hip.lightning import MiniTrainer
    torch.manual_seed(0)
    Net = _net_class()
    base = Net()
    data = _data(3)
    clipped, plain, hand = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    tr = MiniTrainer(max_epochs=1, log_every=1, device="cpu", gradient_clip_val=0.1)
    tr.fit(clipped, train_dataloader=data)
    MiniTrainer(max_epochs=1, log_every=0, device="cpu").fit(plain, train_dataloader=data)
    opt = hand.configure_optimizers()
    norms = []
    for i, batch in enumerate(data):
        hand.training_step(batch, i).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(hand.parameters()), 0.1)))
        opt.step()
        opt.zero_grad()
    assert clipped.global_step == 3
    assert min(norms) > 0.1, "the clip must act for this check to mean anything"
    assert torch.equal(_params(clipped), _params(hand))
    assert not torch.equal(_params(clipped), _params(plain))
    assert clipped.synced_logs()["grad_norm"] == pytest.approx(norms[-1], rel=1e-6)      # logged from the last step


def test_minitrainer_clips_the_accumulated_gradient():
    """K = 2: the clipped norm is the norm of the averaged gradient of two micro-batches; the odd batch is stepped alone"""
    from lgm_hip.lightning import MiniTrainer
    torch.manual_seed(0)
    Net = _net_class()
    base = Net()
    data = _data(3)
    got, hand = copy.deepcopy(base), copy.deepcopy(base)
    MiniTrainer(max_epochs=1, log_every=0, device="cpu", gradient_clip_val=0.1, accumulate_grad_batches=2).fit(
        got, train_dataloader=data)
    opt = hand.configure_optimizers()
    for group in ((0, 1), (2,)):
        for i in group:
            (hand.training_step(data[i], i) / 2).backward()
        torch.nn.utils.clip_grad_norm_(list(hand.parameters()), 0.1)
        opt.step()
        opt.zero_grad()
    assert got.global_step == 2 and torch.equal(_params(got), _params(hand))


def test_minitrainer_refuses_what_it_does_not_build():
    from lgm_hip.lightning import MiniTrainer
    with pytest.raises(ValueError):
        MiniTrainer(device="cpu", gradient_clip_val=0.5, gradient_clip_algorithm="value")
    assert MiniTrainer(device="cpu", gradient_clip_val=0).clip is None and MiniTrainer(device="cpu").clip is None
    Net = _net_class()

    class Manual(Net):
        def __init__(self):
            super().__init__()
            self.automatic_optimization = False

        def training_step(self, batch, batch_idx):
            opt = self.optimizers()
            opt.zero_grad()
            self.manual_backward(super().training_step(batch, batch_idx))
            opt.step()

    data = _data(2)
    for kw in (dict(gradient_clip_val=1.0), dict(accumulate_grad_batches=2)):
        with pytest.raises(ValueError, match="manual"):
            MiniTrainer(max_epochs=1, log_every=0, device="cpu", **kw).fit(Manual(), train_dataloader=data)
    m = Manual()
    MiniTrainer(max_epochs=1, log_every=0, device="cpu").fit(m, train_dataloader=data)      # neither option: trains
    assert m.global_step == 2


def test_fused_optimizers_carry_the_clip_as_an_attribute():
    """max_grad_norm is no param-group entry (state_dict keeps torch's layout); RMSprop refuses it; a slice cannot be
    updated before the whole norm exists"""
    from lgm_hip.optim import FusedAdam, FusedRMSprop
    p = nn.Parameter(torch.zeros(4))
    opt = FusedAdam([p], lr=1e-3, max_grad_norm=1.0)
    assert opt.max_grad_norm == 1.0 and opt.clipping and "max_grad_norm" not in opt.param_groups[0]
    assert FusedAdam([p]).max_grad_norm is None and not FusedAdam([p]).clipping
    with pytest.raises(RuntimeError, match="whole norm"):
        opt.step_slice(None, None, None, 0, 4)
    rms = FusedRMSprop([p])
    assert rms.max_grad_norm is None
    with pytest.raises(ValueError):
        rms.max_grad_norm = 1.0


# ---- host-only queries ------------------------------------------------------------------------------------------------------------

def test_partial_count_is_a_function_of_n_alone():
    from lgm_hip import _lib
    L = _lib.lib()
    span = L.lgm_grad_sqnorm_span(1)
    assert span > 0 and span % 1024 == 0 and L.lgm_grad_sqnorm_span(10 ** 9) == span
    sizes = [1, 2, 1023, span - 1, span, span + 1, 3 * span + 5, 35_700_000, 2 ** 31 + 7]
    counts = [L.lgm_grad_sqnorm_partials(n) for n in sizes]
    assert counts == [(n + span - 1) // span for n in sizes] and counts == sorted(counts)
    assert L.lgm_grad_sqnorm_partials(0) == -1
    base = L.lgm_cu_margin()
    try:
        for margin in (0, 16, 64):
            L.lgm_set_cu_margin(margin)
            assert [L.lgm_grad_sqnorm_partials(n) for n in sizes] == counts
    finally:
        L.lgm_set_cu_margin(-1)
    assert L.lgm_cu_margin() == base


def test_new_entry_points_are_declared_and_reject_bad_arguments_without_a_gpu():
    from lgm_hip import _lib
    L = _lib.lib()
    for name in ("lgm_grad_sqnorm_partial", "lgm_grad_sqnorm_partials", "lgm_grad_clip_scale", "lgm_adam_step_scaled",
                 "lgm_grad_accumulate"):
        assert name in L.protos and hasattr(L._dll, name)
    assert L.lgm_abi_version() == 8
    with pytest.raises(_lib.LgmArgumentError):
        L.lgm_grad_sqnorm_partial(None, 4, None, None)
    with pytest.raises(_lib.LgmArgumentError):
        L.lgm_grad_clip_scale(None, 1, 1.0, 1.0, None, None)
    with pytest.raises(_lib.LgmArgumentError):
        L.lgm_grad_accumulate(None, None, 4, 0, None)
    with pytest.raises(_lib.LgmArgumentError):           # the scale pointer is what this entry point is for
        L.lgm_adam_step_scaled(16, 16, 16, 16, 4, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1.0, None, None, 0, None)
