"""GPU: the self-conditioned DDPM (reference ddpm.py:300-301, 428-435, 899-909 and the x_start handed from step to step of
every sampling loop).

  * the estimate kernel and the slice-aware q_sample / sample-step kernels against float64 restatements (the 8 u M rule of
    tests/test_hip_objectives.py, same shapes), what they must leave untouched, and - called without a self-conditioning
    slice - bit for bit against the plain and ``_obj`` entry points (adapters over the same kernels);
  * UNet output, training step (coin off / on), model_predictions and whole sampling chains against what the REFERENCE's
    ``Unet(self_condition=True)`` / ``GaussianDiffusion`` returned (tests/golden/diffusion_selfcond.npz, written by
    tools/make_golden_selfcond.py), 1e-4 relative; an unclipped x_start or a chain that misses 1e-4 is decided by the float64
    arbiter rule of tests/test_hip_objectives.py (HIP no further from the fixture's float64 evaluation than twice the
    reference is);
  * the gradient of a self-conditioned step flows through the second pass only; ``x_self_cond=None`` is an explicit zero
    tensor; graph replay (sampling chains, training step) bit for bit against eager launches; train.py on
    configs/diffusion/ddpm_selfcond.json.

Measured distances go through the ``parity`` recorder (committed record: profiles/r08_selfcond_parity.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24                        # unit roundoff of float32
KB, KH, KW = 3, 5, 7                  # 105 pixels: a partial last block, no power of two
KT = (0, 517, 999)                    # both ends of the tables
SENTINEL = 7.0
TABLES = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _r4(c):
    return (c + 3) // 4 * 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_selfcond.npz")))


@pytest.fixture(scope="module")
def tables():
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)
    return {n: getattr(gd, n).clone() for n in TABLES}


# ----------------------------------------------------------------------------------------------------------------------
# kernels.  Input buffer [B, HW, pitch], pitch = r4(2 C): C = 3 -> self-conditioning lanes 0..2, x lanes 3..5, padding 6..7;
# C = 1 -> lane 0, lane 1, padding 2..3.  Bounds: every rounding is at most u relative to its partial result and M is the
# sum of the magnitudes of the expression's terms (see tests/test_hip_objectives.py): x_start <= 2 u M, x_t and the target
# <= 3 u M, the sampler update <= 6 u M; asserted against 8 u M.
# ----------------------------------------------------------------------------------------------------------------------
def _within(got, want, bound, what):
    got, want = got.detach().double().cpu(), want.double()
    excess = ((got - want).abs() - 8 * U * bound.double()).max().item()
    assert excess <= 0, f"{what}: error exceeds 8 u M by {excess:.3e}"


def _nchw(buf, lo, C):
    """lanes [lo, lo + C) of a [B, HW, pitch] buffer as a host NCHW tensor"""
    return buf.cpu().reshape(KB, KH, KW, -1)[..., lo:lo + C].permute(0, 3, 1, 2)


def _predictions64(objective, x, out, t, tb, clip, rederive):
    """reference ddpm.py:707-734 in float64 -> (pred_noise, its bound M, x_start, its bound M)"""
    ex = lambda n: tb[n][t].double()[:, None, None, None]  # noqa: E731
    A, S, R, Rm1 = (ex(n) for n in TABLES)
    x, out = x.double(), out.double()
    if objective == 0:
        x0, m0 = R * x - Rm1 * out, (R * x).abs() + (Rm1 * out).abs()
    elif objective == 1:
        x0, m0 = out, out.abs()
    else:
        x0, m0 = A * x - S * out, (A * x).abs() + (S * out).abs()
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    if objective == 0 and not (clip and rederive):
        return out, out.abs(), x0, m0
    pn = (R * x - x0) / Rm1
    return pn, ((R * x).abs() + x0.abs() + m0) / Rm1 + pn.abs(), x0, m0


def _input_buffer(g, C, dev):
    """sentinel everywhere, random x slice -> (device buffer, pitch, x as host NCHW)"""
    pitch = _r4(2 * C)
    buf = torch.full((KB, KH * KW, pitch), SENTINEL)
    buf[..., C:2 * C] = torch.randn(KB, KH * KW, C, generator=g)
    return buf.to(dev), pitch, _nchw(buf, C, C).clone()


def _net_output(g, C, dev):
    v = torch.full((KB, KH * KW, _r4(C)), 3.0)                 # a padded lane of the network output is never used
    v[..., :C] = torch.randn(KB, KH * KW, C, generator=g)
    return v.to(dev), _nchw(v, 0, C).clone()


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("objective", [0, 1, 2], ids=["pred_noise", "pred_x0", "pred_v"])
def test_estimate_kernel(dev, tables, objective, C):
    from lgm_hip import ops
    g = torch.Generator().manual_seed(70 + C)
    xin, pitch, x = _input_buffer(g, C, dev)
    vd, v = _net_output(g, C, dev)
    before = xin.clone()
    t = torch.tensor(KT)
    td, tbd = t.to(dev), [tables[n].to(dev) for n in TABLES]
    ops.lib().lgm_selfcond_estimate(xin.data_ptr(), pitch, C, 0, vd.data_ptr(), _r4(C), td.data_ptr(),
                                    *[b.data_ptr() for b in tbd], objective, KB, C, KH * KW, 1000, ops.stream())
    assert ops.lib()._dll.lgm_last_kernel().decode() == "selfcond_estimate_kernel"
    torch.cuda.synchronize()
    _, _, want, m = _predictions64(objective, x, v, t, tables, 0, 0)
    _within(_nchw(xin, 0, C), want, m, "x_start")
    assert torch.equal(xin[..., C:], before[..., C:]), "the x slice and the pad lanes are not written"
    if objective == 1:
        assert torch.equal(_nchw(xin, 0, C), v)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("with_offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("objective", [0, 1, 2], ids=["pred_noise", "pred_x0", "pred_v"])
def test_qsample_slice_kernel(dev, tables, objective, with_offset, C):
    from lgm_hip import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(40 + C)
    img = torch.rand(KB, C, KH, KW, generator=g)
    noise = torch.randn(KB, C, KH, KW, generator=g)
    off = torch.randn(KB, C, generator=g)
    strength = 0.1
    t = torch.tensor(KT)
    sa, sb = tables["sqrt_alphas_cumprod"], tables["sqrt_one_minus_alphas_cumprod"]
    d = lambda x: x.to(dev).contiguous()  # noqa: E731
    imgd, noised, offd, td, sad, sbd = d(img), d(noise), d(off), d(t), d(sa), d(sb)
    pitch, Cp = _r4(2 * C), _r4(C)
    xin = torch.full((KB, KH * KW, pitch), SENTINEL, device=dev)
    tg = torch.full((KB, KH * KW, Cp), SENTINEL, device=dev)
    L.lgm_qsample_target_slice(imgd.data_ptr(), noised.data_ptr(), offd.data_ptr() if with_offset else None, strength,
                               td.data_ptr(), sad.data_ptr(), sbd.data_ptr(), 1, objective, xin.data_ptr(), pitch, C, 0,
                               tg.data_ptr(), Cp, KB, C, KH * KW, Cp, ops.stream())
    assert L._dll.lgm_last_kernel().decode() == "qsample_slice_kernel"
    torch.cuda.synchronize()
    assert torch.equal(noised.cpu(), noise), "the kernel must not write the caller's noise"
    s32 = float(torch.tensor(strength, dtype=torch.float32))
    a, b = sa[t].double()[:, None, None, None], sb[t].double()[:, None, None, None]
    x0 = img.double() * 2 - 1
    shift = s32 * off.double()[:, :, None, None] if with_offset else torch.zeros(KB, C, 1, 1, dtype=torch.float64)
    n = noise.double() + shift
    n_mag = noise.double().abs() + shift.abs()
    _within(_nchw(xin, C, C), a * x0 + b * n, a * (2 * img.double() + 1) + b * n_mag, "x_t")
    want_tg, m_tg = [(n, n_mag), (x0, 2 * img.double() + 1),
                     (a * n - b * x0, a * n_mag + b * (2 * img.double() + 1))][objective]
    _within(_nchw(tg, 0, C), want_tg, m_tg, "target")
    assert float(xin[..., :C].abs().max()) == 0, "the self-conditioning slice is zeroed in the same launch"
    assert float(xin[..., 2 * C:].abs().max()) == 0 and float(tg[..., C:].abs().max() if Cp > C else 0) == 0, \
        "pad lanes are written as zero"
    # the target is the existing entry point's, bit for bit, and so is x_t
    xt2 = torch.full((KB, KH * KW, Cp), SENTINEL, device=dev)
    tg2 = torch.full_like(tg, SENTINEL)
    L.lgm_qsample_target_obj(imgd.data_ptr(), noised.data_ptr(), offd.data_ptr() if with_offset else None, strength,
                             td.data_ptr(), sad.data_ptr(), sbd.data_ptr(), 1, objective, xt2.data_ptr(), tg2.data_ptr(),
                             Cp, KB, C, KH * KW, Cp, ops.stream())
    assert torch.equal(tg, tg2) and torch.equal(xin[..., C:2 * C], xt2[..., :C])


@pytest.mark.parametrize("C", [3, 1])
def test_sample_step_slice_kernels(dev, tables, C):
    """x from its slice, the next x into the slice of the other buffer, the handed-on x0 (clipped when clip is set) into the
    self-conditioning slice; the table-driven in-place form gives the by-value form's bits."""
    from lgm_hip import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(60 + C)
    HW = KH * KW
    xin, pitch, x = _input_buffer(g, C, dev)
    vd, v = _net_output(g, C, dev)
    nz = torch.randn(KB, C, KH, KW, generator=g)
    nzd = nz.to(dev)
    tq = 517
    A, Bv = float(tables["sqrt_alphas_cumprod"][tq]), -float(tables["sqrt_one_minus_alphas_cumprod"][tq])
    R, Rm1 = float(tables["sqrt_recip_alphas_cumprod"][tq]), float(tables["sqrt_recipm1_alphas_cumprod"][tq])
    C0, C1, C2, C3 = 0.75, 0.125, 0.5, 0.25
    table = torch.tensor([[0.0] * 8, [A, Bv, R, Rm1, C0, C1, C2, C3]], device=dev)
    counter = torch.ones(1, dtype=torch.int32, device=dev)
    tb = {k: b[tq:tq + 1].expand(KB).contiguous() for k, b in tables.items()}
    tzero = torch.zeros(KB, dtype=torch.long)
    for objective in (0, 1, 2):
        for clip, red in ((1, 0), (1, 1), (0, 0)):
            out = torch.full_like(xin, SENTINEL)
            L.lgm_sample_step_slice(xin.data_ptr(), out.data_ptr(), pitch, C, 0, vd.data_ptr(), _r4(C), nzd.data_ptr(), KB, C,
                                    HW, objective, A, Bv, clip, red, R, Rm1, C0, C1, C2, C3, ops.stream())
            assert L._dll.lgm_last_kernel().decode() == "sample_step_slice_kernel"
            xi = xin.clone()
            L.lgm_sample_step_table_slice(xi.data_ptr(), pitch, C, 0, vd.data_ptr(), _r4(C), nzd.data_ptr(), KB, C, HW,
                                          table.data_ptr(), counter.data_ptr(), objective, clip, red, 0, ops.stream())
            assert torch.equal(xi, out), (objective, clip, red)
            assert int(counter) == 1
            assert float(out[..., 2 * C:].abs().max()) == 0, "pad lanes are written as zero"
            pn, m_pn, xs, m_xs = _predictions64(objective, x, v, tzero, tb, clip, red)
            _within(_nchw(out, 0, C), xs, m_xs, "x0 handed on")
            if clip:
                assert float(out[..., :C].abs().max()) <= 1.0
            want = C0 * xs + C1 * x.double() + C2 * pn + C3 * nz.double()
            _within(_nchw(out, C, C), want, C0 * m_xs + C1 * x.double().abs() + C2 * m_pn + C3 * nz.double().abs(), "update")
    L.lgm_sample_step_table_slice(xi.data_ptr(), pitch, C, 0, vd.data_ptr(), _r4(C), None, KB, C, HW, table.data_ptr(),
                                  counter.data_ptr(), 0, 1, 0, 1, ops.stream())
    assert int(counter) == 2                                   # advance != 0 appends counter += 1


@pytest.mark.parametrize("C", [3, 1])
def test_slice_forms_without_self_conditioning_equal_the_existing_entry_points(dev, tables, C):
    """pitch = r4(C), x offset 0, no self-conditioning slice: the bits of lgm_qsample_target[_obj], lgm_sample_step[_obj] and
    lgm_sample_step_table[_obj], pad lanes included."""
    from lgm_hip import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(80 + C)
    HW, Cp = KH * KW, _r4(C)
    img = torch.rand(KB, C, KH, KW, generator=g).to(dev)
    noise = torch.randn(KB, C, KH, KW, generator=g).to(dev)
    off = torch.randn(KB, C, generator=g).to(dev)
    td = torch.tensor(KT).to(dev)
    sad, sbd = tables["sqrt_alphas_cumprod"].to(dev), tables["sqrt_one_minus_alphas_cumprod"].to(dev)
    new = lambda: torch.full((KB, HW, Cp), SENTINEL, device=dev)  # noqa: E731
    for objective in (0, 1, 2):
        for o in (None, off):
            a, ta, b, tb_ = new(), new(), new(), new()
            op = None if o is None else o.data_ptr()
            L.lgm_qsample_target_slice(img.data_ptr(), noise.data_ptr(), op, 0.1, td.data_ptr(), sad.data_ptr(),
                                       sbd.data_ptr(), 1, objective, a.data_ptr(), Cp, 0, -1, ta.data_ptr(), Cp, KB, C, HW, Cp,
                                       ops.stream())
            L.lgm_qsample_target_obj(img.data_ptr(), noise.data_ptr(), op, 0.1, td.data_ptr(), sad.data_ptr(), sbd.data_ptr(), 1,
                                     objective, b.data_ptr(), tb_.data_ptr(), Cp, KB, C, HW, Cp, ops.stream())
            assert torch.equal(a, b) and torch.equal(ta, tb_), (objective, o is not None)
            if objective == 2 and o is None:
                b, tb_ = new(), new()
                L.lgm_qsample_target(img.data_ptr(), noise.data_ptr(), td.data_ptr(), sad.data_ptr(), sbd.data_ptr(), 1,
                                     b.data_ptr(), tb_.data_ptr(), Cp, KB, C, HW, Cp, ops.stream())
                assert torch.equal(a, b) and torch.equal(ta, tb_)
    x = torch.zeros(KB, HW, Cp)
    x[..., :C] = torch.randn(KB, HW, C, generator=g)
    xd = x.to(dev)
    vd, _ = _net_output(g, C, dev)
    tq = 517
    A, Bv = float(tables["sqrt_alphas_cumprod"][tq]), -float(tables["sqrt_one_minus_alphas_cumprod"][tq])
    R, Rm1 = float(tables["sqrt_recip_alphas_cumprod"][tq]), float(tables["sqrt_recipm1_alphas_cumprod"][tq])
    C0, C1, C2, C3 = 0.75, 0.125, 0.5, 0.25
    table = torch.tensor([[0.0] * 8, [A, Bv, R, Rm1, C0, C1, C2, C3]], device=dev)
    counter = torch.ones(1, dtype=torch.int32, device=dev)
    for objective in (0, 1, 2):
        for clip, red in ((1, 0), (1, 1), (0, 0)):
            a, b = new(), new()
            L.lgm_sample_step_slice(xd.data_ptr(), a.data_ptr(), Cp, 0, -1, vd.data_ptr(), Cp, noise.data_ptr(), KB, C, HW,
                                    objective, A, Bv, clip, red, R, Rm1, C0, C1, C2, C3, ops.stream())
            L.lgm_sample_step_obj(xd.data_ptr(), vd.data_ptr(), noise.data_ptr(), b.data_ptr(), None, KB, C, HW, Cp, objective, A,
                                  Bv, clip, red, R, Rm1, C0, C1, C2, C3, ops.stream())
            assert torch.equal(a, b), (objective, clip, red)
            ai, bi = xd.clone(), xd.clone()
            L.lgm_sample_step_table_slice(ai.data_ptr(), Cp, 0, -1, vd.data_ptr(), Cp, noise.data_ptr(), KB, C, HW,
                                          table.data_ptr(), counter.data_ptr(), objective, clip, red, 0, ops.stream())
            L.lgm_sample_step_table_obj(bi.data_ptr(), vd.data_ptr(), noise.data_ptr(), None, KB, C, HW, Cp, table.data_ptr(),
                                        counter.data_ptr(), objective, clip, red, 0, ops.stream())
            assert torch.equal(ai, bi) and torch.equal(ai, a)
            if objective == 2:
                b, bi = new(), xd.clone()
                L.lgm_sample_step(xd.data_ptr(), vd.data_ptr(), noise.data_ptr(), b.data_ptr(), None, KB, C, HW, Cp, A, Bv, clip,
                                  R, Rm1, C0, C1, C2, C3, ops.stream())
                L.lgm_sample_step_table(bi.data_ptr(), vd.data_ptr(), noise.data_ptr(), None, KB, C, HW, Cp, table.data_ptr(),
                                        counter.data_ptr(), clip, 0, ops.stream())
                assert torch.equal(a, b) and torch.equal(ai, bi)


# ----------------------------------------------------------------------------------------------------------------------
# parity with the reference's self-conditioned Unet / GaussianDiffusion (dim 16, 16 x 16, B = 2, t = (37, 912))
# ----------------------------------------------------------------------------------------------------------------------
class _Case:
    def __init__(self, fx, objective, dev):
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        from oracle import diffusion as OD
        self.o, self.dev = objective, dev
        self.dim, self.S, self.B = int(fx["dim"]), int(fx["S"]), int(fx["B"])
        self.P = OD.unet_init(dim=self.dim, channels=3, seed=int(fx["seed"]))
        self.P["init_conv.weight"] = torch.as_tensor(fx["init_conv.weight"])
        g = torch.Generator().manual_seed(int(fx["data_seed"]))
        self.img = torch.rand(self.B, 3, self.S, self.S, generator=g)
        self.noise = torch.randn(self.B, 3, self.S, self.S, generator=g)
        self.t = torch.as_tensor(fx["t"])
        self.sc = torch.as_tensor(fx["x_self_cond"])
        self.net = Unet(dim=self.dim, channels=3, self_condition=True)
        self.net.load_state_dict(self.P, strict=True)
        self.gd = GaussianDiffusion(self.net, img_size=self.S, timesteps=1000, sampling_timesteps=int(fx["ddim_steps"]),
                                    objective=objective).to(dev)
        self.net.prepare_hip(dev)
        self.fx = {k[len(objective) + 1:]: v for k, v in fx.items() if k.startswith(objective + ":")}
        self.x_t = torch.as_tensor(self.fx["x_t"])


@pytest.fixture(scope="module", params=["pred_v", "pred_noise"])
def case(request, fx, dev):
    return _Case(fx, request.param, dev)


def _arbiter(parity, what, hip, ref, exact=None):
    """1e-4 against the reference's fp32 result; with ``exact`` (the fixture's float64 evaluation: sampling chains and the
    unclipped x_start only) a miss is decided by float64 - HIP no further from it than twice the reference itself."""
    e = rel(hip, ref)
    if e < RTOL or exact is None:
        return parity(what, e, RTOL)
    d_ref, d_hip = rel(ref, exact), rel(hip, exact)
    parity.record(what + " [float64 arbiter]", hip_vs_ref=e, ref_vs_fp64=d_ref, hip_vs_fp64=d_hip)
    print(f"[parity] {what}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, hip {d_hip:.3e}")
    assert d_hip <= 2 * d_ref, (what, e, d_hip, d_ref)


def test_unet_output_matches_reference_fixture(case, parity):
    net, dev = case.net, case.dev
    x, t = case.x_t.to(dev), case.t.to(dev)
    with torch.no_grad():
        with_sc, none = net(x, t, case.sc.to(dev)), net(x, t)
        zeros = net(x, t, torch.zeros_like(x))
    parity(f"{case.o}: unet_out, supplied x_self_cond", rel(with_sc, case.fx["unet_out:sc"]), RTOL)
    parity(f"{case.o}: unet_out, x_self_cond=None", rel(none, case.fx["unet_out:none"]), RTOL)
    assert torch.equal(none, zeros), "x_self_cond=None is an explicit zero tensor"
    assert rel(with_sc, none) > 1e-2, "the self-conditioning input reaches the output"
    mp_none = case.gd.model_predictions(x, t)
    mp_zero = case.gd.model_predictions(x, t, torch.zeros_like(x))
    assert torch.equal(mp_none.pred_x_start, mp_zero.pred_x_start) and torch.equal(mp_none.pred_noise, mp_zero.pred_noise)


def _grad_checks(parity, case, pre, tag):
    fx, net = case.fx, case.net
    sd = dict(net.named_parameters())
    worst, worst_n, worst_s, n_seen = 0.0, 0.0, 0.0, 0
    K = 1024
    for k in fx:
        if k.startswith(pre + "grad:"):
            worst = max(worst, rel(sd[k[len(pre) + 5:]].grad, fx[k]))
            n_seen += 1
        elif k.startswith(pre + "gradnorm:"):
            n = k[len(pre) + 9:]
            worst_n = max(worst_n, abs(sd[n].grad.double().norm().item() - float(fx[k])) / max(float(fx[k]), 1e-12))
            flat = sd[n].grad.reshape(-1)
            worst_s = max(worst_s, rel(flat[:: flat.numel() // K][:K], fx[pre + "gradsample:" + n]))
            n_seen += 1
    assert n_seen == 26
    assert sd["init_conv.weight"].grad.shape == (16, 6, 7, 7)
    parity(f"{case.o}{tag}: init_conv.weight gradient [16, 6, 7, 7]",
           rel(sd["init_conv.weight"].grad, fx[pre + "grad:init_conv.weight"]), RTOL)
    parity(f"{case.o}{tag}: worst parameter gradient (23 whole tensors)", worst, RTOL)
    parity(f"{case.o}{tag}: worst gradient norm (3 large tensors)", worst_n, RTOL)
    parity(f"{case.o}{tag}: worst 1024-element gradient sample (3 large tensors)", worst_s, RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    want = float(fx[pre + "gradnorm_all"])
    parity(f"{case.o}{tag}: all-parameter gradient norm", abs(gn - want) / want, RTOL)


@pytest.mark.parametrize("coin", [False, True], ids=["coin_off", "coin_on"])
def test_training_step_matches_reference_fixture(case, parity, coin):
    gd, net, dev = case.gd, case.net, case.dev
    pre = f"coin{int(coin)}:"
    x0 = (case.img * 2 - 1).to(dev)
    noise = case.noise.to(dev)
    net._flat.zero_grad()
    loss = gd.p_losses(x0, case.t.to(dev), noise, _self_cond=coin)
    assert torch.equal(noise.cpu(), case.noise)
    want = float(case.fx[pre + "loss"])
    parity(f"{case.o}, coin {int(coin)}: loss", abs(loss.item() - want) / want, RTOL)
    assert abs(float(case.fx["coin1:loss"]) - float(case.fx["coin0:loss"])) / want > RTOL, "the coin moves the reference's loss"
    loss.backward()
    _grad_checks(parity, case, pre, f", coin {int(coin)}")


def test_the_default_coin_is_pythons_random(case, monkeypatch):
    """without an injected value the coin is ``random.random() < 0.5`` (reference :902)"""
    from models.generative.diffusion import ddpm
    gd, dev = case.gd, case.dev
    x0, t, noise = (case.img * 2 - 1).to(dev), case.t.to(dev), case.noise.to(dev)
    with torch.no_grad():
        off, on = gd.p_losses(x0, t, noise, _self_cond=False), gd.p_losses(x0, t, noise, _self_cond=True)
        monkeypatch.setattr(ddpm.random, "random", lambda: 0.75)
        assert torch.equal(gd.p_losses(x0, t, noise), off)
        monkeypatch.setattr(ddpm.random, "random", lambda: 0.25)
        assert torch.equal(gd.p_losses(x0, t, noise), on)
    assert not torch.equal(on, off)


def test_gradient_flows_through_the_second_pass_only(case):
    """p_losses(_self_cond=True) against the two-call run: the estimate from model_predictions, fed to the same loss as a
    constant.  Loss and every gradient bit-equal."""
    gd, net, dev = case.gd, case.net, case.dev
    x0, t, noise = (case.img * 2 - 1).to(dev), case.t.to(dev), case.noise.to(dev)
    net._flat.zero_grad()
    la = gd.p_losses(x0, t, noise, _self_cond=True)
    la.backward()
    ga = {n: p.grad.clone() for n, p in net.named_parameters()}
    est = gd.model_predictions(gd.q_sample(x0, t, noise), t).pred_x_start
    assert float(est.abs().max()) > 1.0, "the estimate is not clipped (clip_x_start=False, reference :904)"
    net._flat.zero_grad()
    lb = gd.p_losses(x0, t, noise, _self_cond=est)
    lb.backward()
    assert torch.equal(la, lb), (float(la), float(lb))
    for n, p in net.named_parameters():
        assert torch.equal(ga[n], p.grad), n


@pytest.mark.parametrize("clip", [False, True])
def test_model_predictions_match_reference_fixture(case, parity, clip):
    dev = case.dev
    x, t, sc = case.x_t.to(dev), case.t.to(dev), case.sc.to(dev)
    pred = case.gd.model_predictions(x, t, sc, clip_x_start=clip)
    key = f"mp:{int(clip)}:"
    _arbiter(parity, f"{case.o}: pred_noise, clip={clip}", pred.pred_noise, case.fx[key + "pred_noise"])
    _arbiter(parity, f"{case.o}: pred_x_start, clip={clip}", pred.pred_x_start, case.fx[key + "x_start"],
             None if clip else case.fx["mp:0:x_start64"])
    if clip:                                                   # p_mean_variance (:736-746) and p_sample take x_self_cond too
        mean, _, _, xs = case.gd.p_mean_variance(x, t, sc, clip_denoised=True)
        assert torch.equal(xs, pred.pred_x_start) and torch.isfinite(mean).all()
        nz = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        img_a, xs_a = case.gd.p_sample(x, 500, sc, noise=nz)
        img_b, xs_b = case.gd.p_sample(x, 500, None, noise=nz)
        assert float(xs_a.abs().max()) <= 1.0 and not torch.equal(img_a, img_b) and not torch.equal(xs_a, xs_b)


def _chains(case, fx, dev):
    """the three chains of the fixture on the HIP engine -> {name: image}"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion
    from oracle import diffusion as OD
    gd = case.gd
    shape = tuple(case.x_t.shape)
    n = int(fx["ddim_steps"])
    out = {}
    init, nz = OD.draw_loop_noise(int(fx["ddim_loop_seed"]), shape, n - 1)
    out["ddim_loop"] = sampler.ddim_sample(gd, shape, init_noise=init.to(dev), noises=[x.to(dev) for x in nz] + [None]).clone()
    gd_e = GaussianDiffusion(case.net, img_size=case.S, timesteps=1000, sampling_timesteps=n, objective=case.o,
                             ddim_sampling_eta=float(fx["eta"])).to(dev)
    init, nz = OD.draw_loop_noise(int(fx["ddim_eta_loop_seed"]), shape, n - 1)
    out["ddim_eta_loop"] = sampler.ddim_sample(gd_e, shape, init_noise=init.to(dev),
                                               noises=[x.to(dev) for x in nz] + [None]).clone()
    T = int(fx["ancestral_T"])
    gd_a = GaussianDiffusion(case.net, img_size=case.S, timesteps=T, objective=case.o).to(dev)
    init, nz = OD.draw_loop_noise(int(fx["p_sample_loop_seed"]), shape, T - 1)
    out["p_sample_loop"] = sampler.p_sample_loop(gd_a, shape, init_noise=init.to(dev),
                                                 noises=[x.to(dev) for x in nz] + [None]).clone()
    return out


def test_sampling_chains_match_reference_fixture_and_graph_replay_equals_eager(case, fx, parity, monkeypatch):
    from lgm_hip import sampler
    dev = case.dev
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = _chains(case, fx, dev)
    per = sampler._GRAPHS[case.net]
    assert len(per) >= 2 and all(isinstance(e, sampler._GraphedChain) for e in per.values()), "graph capture did not happen"
    again = _chains(case, fx, dev)                             # a second chain on the same captured steps: the slice is re-zeroed
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = _chains(case, fx, dev)
    for k, what in (("ddim_loop", "50-pair DDIM chain, eta = 0"), ("ddim_eta_loop", "50-pair DDIM chain, eta = 0.7"),
                    ("p_sample_loop", "200-step ancestral chain")):
        assert torch.isfinite(graph[k]).all() and float(graph[k].std()) > 0
        assert torch.equal(graph[k], eager[k]), f"{what}: graph replay differs from eager launches"
        assert torch.equal(graph[k], again[k]), f"{what}: the second chain on one captured step differs from the first"
        _arbiter(parity, f"{case.o}: {what}, final image", graph[k], case.fx[k], case.fx[k + "64"])


def test_interpolate_and_sample_run_self_conditioned(case):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    dev = case.dev
    gd_a = GaussianDiffusion(case.net, img_size=case.S, timesteps=6, objective=case.o).to(dev)
    x1, x2 = torch.rand(2, 3, 16, 16, device=dev) * 2 - 1, torch.rand(2, 3, 16, 16, device=dev) * 2 - 1
    assert torch.isfinite(gd_a.interpolate(x1, x2, t=4)).all()
    out = gd_a.sample(batch_size=2, return_all_timesteps=True)
    assert out.shape == (2, 7, 3, 16, 16) and torch.isfinite(out).all()


def test_one_channel_network_matches_reference_fixture(fx, dev, parity):
    """channels = 1: input pitch 4, the self-conditioning slice is lane 0 and the x slice lane 1"""
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    P = OD.unet_init(dim=16, channels=1, seed=int(fx["c1_seed"]))
    P["init_conv.weight"] = torch.as_tensor(fx["c1:init_conv.weight"])
    net = Unet(dim=16, channels=1, self_condition=True)
    net.load_state_dict(P, strict=True)
    gd = GaussianDiffusion(net, img_size=16, timesteps=1000, objective="pred_v").to(dev)
    net.prepare_hip(dev)
    assert (net.in_pitch, net.x_off, net.sc_off) == (4, 1, 0)
    g = torch.Generator().manual_seed(int(fx["data_seed"]))
    img = torch.rand(2, 3, 16, 16, generator=g)
    noise = torch.randn(2, 3, 16, 16, generator=g)
    x0, n1 = (img * 2 - 1)[:, :1].contiguous().to(dev), noise[:, :1].contiguous().to(dev)
    sc = torch.as_tensor(fx["x_self_cond"])[:, :1].contiguous().to(dev)
    t = torch.as_tensor(fx["t"]).to(dev)
    with torch.no_grad():
        out = net(gd.q_sample(x0, t, n1), t, sc)
        loss = gd.p_losses(x0, t, n1, _self_cond=True)
    parity("one channel: unet_out, supplied x_self_cond", rel(out, fx["c1:unet_out:sc"]), RTOL)
    want = float(fx["c1:coin1:loss"])
    parity("one channel: loss, coin on", abs(loss.item() - want) / want, RTOL)


# ----------------------------------------------------------------------------------------------------------------------
# the graph-replayed training step against eager steps, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def _module(dev, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(img_size=16, dim=16, lr=1e-3, self_condition=True, ema_update_every=2, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("kw", [dict(), dict(objective="pred_noise", offset_noise_strength=0.1)], ids=["pred_v", "pred_noise_offset"])
def test_graph_replayed_training_step_equals_eager_steps(dev, kw):
    """Six steps with the coin sequence off, on, on, off, on, off through ``make_fast_step``: losses, parameters after Adam,
    the EMA shadow (updated every second step here) and the Adam state of graph replay and eager launches are the same bits."""
    coins = [False, True, True, False, True, False]
    a, b = _module(dev, **kw), _module(dev, **kw)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True), b.make_fast_step(ob, 1, False)
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(4, 3, 16, 16, generator=g).to(dev) for _ in coins]
    losses = {}
    for name, fast in (("graph", fa), ("eager", fb)):
        torch.manual_seed(77)                                  # the device generator: same draws in both runs
        fast.coin = iter(coins).__next__
        losses[name] = [fast.step((x.clone(), None), i).detach().clone().reshape(()) for i, x in enumerate(xs)]
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    assert fa.graphed.pre is not None and fa.graphed.est is not None
    for la, lb in zip(losses["graph"], losses["eager"]):
        assert torch.isfinite(la) and torch.equal(la, lb), (float(la), float(lb))
    assert len({float(x) for x in losses["graph"]}) == len(coins)
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data)
    ea, eb = a.ema.ema_model.model, b.ema.ema_model.model
    assert torch.equal(ea._flat.data, eb._flat.data)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    for pa, pb in zip(oa.state_dict()["state"].values(), ob.state_dict()["state"].values()):
        for k in pb:
            assert torch.equal(torch.as_tensor(pa[k]), torch.as_tensor(pb[k])), k


def test_train_entry_runs_the_selfcond_config(tmp_path):
    """python train.py --config_path <configs/diffusion/ddpm_selfcond.json at a reduced size> --max_steps 3: 16 x 16, dim 16
    and 50 diffusion steps (the step-0 sample is then a 50-step self-conditioned ancestral chain)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "ddpm_selfcond.json")))
    assert cfg["model"]["args"]["self_condition"] is True
    cfg["model"]["args"].update(img_size=16, dim=16, diffusion_timesteps=50)
    cfg["dataset"].update(img_size=16, batch_size=8)
    path = tmp_path / "ddpm_selfcond_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_ddpm_selfcond"
    cmd = [sys.executable, os.path.join(pkg, "train.py"), "--config_path", str(path), "--max_steps", "3", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 3 and sd["hyper_parameters"]["self_condition"] is True
    w = sd["state_dict"]["ema.online_model.model.init_conv.weight"]
    assert tuple(w.shape) == (16, 6, 7, 7)
    for v in sd["state_dict"].values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
