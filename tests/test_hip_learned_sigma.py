"""GPU: the learned-variance DDPM on the HIP path (Nichol & Dhariwal 2021): ``Unet(learned_variance=True)``, the hybrid loss
(``lgm_hybrid_loss_fwd`` / ``_bwd``), the ancestral step with the learned variance (``lgm_sample_step_learned`` /
``_table_learned``) and the bound with it (``vlb_terms(variance="learned")``, ``lgm_vlb_term_learned``).

  (a) the narrow 1x1 kernels at Nw = 8 (the final_conv 64 -> 6 and its input gradient) against float64 elementwise, in the
      direct-convolution ledger's units (oracle/bounds.py: 2^-24 S per element, ``bounds.tolerance`` of the reduction length:
      64 forward, 6 for the input gradient), at P = 1, 63, 65 and 2048 * 64 + 17 pixels (one pixel row past the grid cap);
  (b) the loss kernels alone against float64 (torch.float64 autograd of the textbook formulas from the same float32 operands
      and tables): B = 3 with t = (0, 1, T - 1), C = 3 / 1 at HW = 25, v in [-3, 3], residuals up to +-9 sigma at t = 0, x0 on both
      end bins.  Per-sample terms at the project's 1e-4; the prediction lanes of the gradient equal lgm_weighted_mse_bwd's
      bits; the variance lanes within twice the distance the fixture's own float32 autograd has from float64 ("gvar_dist",
      tools/make_golden_learned_sigma.py) - a fixed-order float32 evaluation may round differently, not worse in kind;
  (c) - (d) parity with tests/golden/diffusion_learned_sigma.npz at its B = 4, T = 8 on the small network: loss, per-sample
      terms, output gradient, every parameter gradient; p_sample at t = 0, 1, 7; the bound over all 8 timesteps.  1e-4
      relative against float64 (tests/test_hip_objectives.py, tests/test_hip_bpd.py), a parameter gradient that misses it
      decided by the arbiter rule of those files: no further from float64 than twice the float32 reference ("dref:<name>");
  (e) graph replay against eager launches, bit for bit: one DDPMFastStep step, the ancestral chain, the likelihood loop;
  (f) DDIM and DPM-Solver++ on the learned-variance network equal the chain of a plain network holding the prediction rows of
      its final_conv, bit for bit; a guided forward leaves the variance lanes the conditional forward's.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import bounds

pytestmark = pytest.mark.gpu
RTOL = 1e-4
NAN = float("nan")
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_learned_sigma.npz")))


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _r4(n):
    return (n + 3) // 4 * 4


def _last():
    from lgm_hip import ops
    return ops.lib()._dll.lgm_last_kernel().decode()


# ----------------------------------------------------------------------------------------------------------------------
# (a) narrow 1x1 kernels, Nw = 8
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow_ref():
    """one reference for every P: operands of the largest, prefixes for the others"""
    P = 2048 * 64 + 17
    g = torch.Generator().manual_seed(6408)
    return dict(x=torch.randn(P, 64, generator=g), w=torch.randn(6, 64, generator=g) / 8.0, b=torch.randn(6, generator=g),
                gy=torch.randn(P, 6, generator=g))


@pytest.mark.parametrize("P", [1, 63, 65, 2048 * 64 + 17])
def test_narrow1x1_nw8_forward_and_input_gradient(dev, narrow_ref, parity, P):
    from lgm_hip import ops
    r = narrow_ref
    x, gy, w, b = r["x"][:P], r["gy"][:P], r["w"], r["b"]
    geom = ops.make_geom(1, 1, P, 64, 8, 1, 1, 1, 0)
    wd = torch.zeros(8, 1, 64)
    wd[:6, 0] = w
    bd = torch.zeros(8)
    bd[:6] = b
    wd, bd = wd.to(dev), bd.to(dev)
    xd = x.to(dev).reshape(1, 1, P, 64).contiguous()
    ybuf = torch.full((1, 1, P + 2, 8), NAN, device=dev)          # a guard pixel on either side
    y = ybuf[:, :, 1:P + 1]
    ops.conv_xy(geom, xd, wd.data_ptr(), bd.data_ptr(), None, y)
    assert _last() == "narrow1x1_fwd_kernel"
    gyd = torch.zeros(1, 1, P, 8, device=dev)
    gyd[0, 0, :, :6] = gy.to(dev)
    gbuf = torch.full((1, 1, P + 2, 64), NAN, device=dev)
    gx = gbuf[:, :, 1:P + 1]
    ops.conv_yx(geom, gyd, wd.data_ptr(), None, None, gx)
    assert _last() == "narrow1x1_dgrad_kernel"
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[0, 0, 0]).all() and torch.isnan(ybuf[0, 0, P + 1]).all(), "forward wrote outside its pixels"
    assert torch.isnan(gbuf[0, 0, 0]).all() and torch.isnan(gbuf[0, 0, P + 1]).all(), "input gradient wrote outside its pixels"
    x64, w64, b64, g64 = x.double(), w.double(), b.double(), gy.double()
    want = torch.zeros(P, 8, dtype=torch.float64)
    S = torch.zeros(P, 8, dtype=torch.float64)
    want[:, :6] = x64 @ w64.T + b64
    S[:, :6] = x64.abs() @ w64.abs().T + b64.abs()
    e = bounds.forward_error_units(y.reshape(P, 8), want, S)
    parity(f"narrow1x1 Nw = 8 forward, P = {P}: worst element in units of 2^-24 S", e, bounds.tolerance(64))
    e = bounds.forward_error_units(gx.reshape(P, 64), g64 @ w64, g64.abs() @ w64.abs())
    parity(f"narrow1x1 Nw = 8 input gradient, P = {P}: worst element in units of 2^-24 S", e, bounds.tolerance(6))


# ----------------------------------------------------------------------------------------------------------------------
# (b) the loss kernels alone
# ----------------------------------------------------------------------------------------------------------------------
def approx_cdf(z):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def decoder_ll(x, mean, log_scale):
    """the discretised Gaussian log-likelihood in its textbook form (Nichol & Dhariwal 2021)"""
    inv = torch.exp(-log_scale)
    cdf_plus, cdf_min = approx_cdf(inv * (x - mean + 1.0 / 255.0)), approx_cdf(inv * (x - mean - 1.0 / 255.0))
    log_plus = torch.log(cdf_plus.clamp(min=1e-12))
    log_one_minus = torch.log((1.0 - cdf_min).clamp(min=1e-12))
    log_delta = torch.log((cdf_plus - cdf_min).clamp(min=1e-12))
    return torch.where(x < -0.999, log_plus, torch.where(x > 0.999, log_one_minus, log_delta))


def learned_terms64(tab, t, x0, xt, x0p, v):
    """per-element term in nats, float64, from [T, 8] table rows; every operand [B, ...] with t [B]"""
    row = lambda k: tab[t][:, k].reshape(-1, *((1,) * (x0.dim() - 1)))  # noqa: E731
    f = (v + 1) / 2
    lv = f * row(0) + (1 - f) * row(1)
    mean = row(3) * x0p + row(4) * xt
    d = row(3) * (x0p - x0)
    kl = 0.5 * (-1.0 + lv - row(2) + torch.exp(row(2) - lv) + d * d * torch.exp(-lv))
    dec = -decoder_ll(x0, mean, 0.5 * lv)
    return torch.where((t == 0).reshape(-1, *((1,) * (x0.dim() - 1))), dec, kl)


@pytest.fixture(scope="module")
def gvar_bound(fx):
    """twice the distance of the fixture's float32 autograd evaluation of the variance-lane gradient from its float64 one"""
    return 2.0 * float(fx["gvar_dist"])


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_hybrid_loss_kernels_against_float64(dev, parity, gvar_bound, objective, C):
    from lgm_hip import ops
    from models.generative.diffusion.ddpm import OBJECTIVES, GaussianDiffusion, Unet
    T, B, HW, W_VB = 8, 3, 25, 0.37
    gd = GaussianDiffusion(Unet(dim=16, channels=C, learned_variance=True), img_size=5, timesteps=T, objective=objective,
                           beta_schedule="cosine", vb_loss_weight=W_VB)
    t = torch.tensor([0, 1, T - 1])
    g = torch.Generator().manual_seed(6500 + C)
    pitch, tpitch, xpitch = _r4(2 * C), _r4(C), _r4(C)
    img = torch.randint(1, 255, (B, C, HW), generator=g).float() / 255.0
    img[0, 0, 0], img[0, 0, 1], img[0, C - 1, 2], img[0, C - 1, 3] = 0.0, 1.0, 0.0, 1.0      # both end bins at t = 0
    x0 = img * 2 - 1
    noise = torch.randn(B, C, HW, generator=g)
    sa, s1 = gd.sqrt_alphas_cumprod[t][:, None, None], gd.sqrt_one_minus_alphas_cumprod[t][:, None, None]
    R, Rm1 = gd.sqrt_recip_alphas_cumprod[t][:, None, None], gd.sqrt_recipm1_alphas_cumprod[t][:, None, None]
    xt = sa * x0 + s1 * noise
    v = torch.rand(B, C, HW, generator=g) * 6 - 3
    tab = gd.learned_table.clone()
    # residuals: sample 0 (t = 0) sweeps x0_pred - x0 over [-9, 9] sigma of the element, the others are O(1)
    f = (v + 1) / 2
    sigma = torch.exp(0.5 * (f * tab[t][:, 0, None, None] + (1 - f) * tab[t][:, 1, None, None]))
    resid = torch.randn(B, C, HW, generator=g)
    resid[0] = torch.linspace(-9, 9, C * HW).reshape(C, HW)[:, torch.randperm(HW, generator=g)] * sigma[0]
    x0p = x0 + resid
    pred = {"pred_x0": x0p, "pred_v": (sa * xt - x0p) / s1, "pred_noise": (R * xt - x0p) / Rm1}[objective]
    target = {"pred_x0": x0, "pred_v": sa * noise - s1 * x0, "pred_noise": noise}[objective]
    nhwc = lambda a: a.permute(0, 2, 1)  # noqa: E731
    out = torch.full((B, HW, pitch), NAN)
    out[..., :C], out[..., C:2 * C] = nhwc(pred), nhwc(v)
    tg = torch.full((B, HW, tpitch), NAN)
    tg[..., :C] = nhwc(target)
    xin = torch.full((B, HW, xpitch), NAN)
    xin[..., :C] = nhwc(xt)
    d = lambda a: a.to(dev).contiguous()  # noqa: E731
    outd, tgd, xind, imgd, td, gdd = d(out), d(tg), d(xin), d(img), d(t), gd.to(dev)
    gl = torch.tensor([1.7], device=dev)
    per = torch.full((2, B), NAN, device=dev)
    loss = torch.full((1,), NAN, device=dev)
    gout = torch.full((B, HW, pitch), NAN, device=dev)
    L = ops.lib()
    head = (outd.data_ptr(), pitch, tgd.data_ptr(), tpitch, imgd.data_ptr(), 1, xind.data_ptr(), xpitch, 0, td.data_ptr(),
            gdd.sqrt_alphas_cumprod.data_ptr(), gdd.sqrt_one_minus_alphas_cumprod.data_ptr(),
            gdd.sqrt_recip_alphas_cumprod.data_ptr(), gdd.sqrt_recipm1_alphas_cumprod.data_ptr(), gdd.loss_weight.data_ptr(),
            gdd.learned_table.data_ptr(), T, OBJECTIVES[objective], W_VB)
    L.lgm_hybrid_loss_fwd(*head, B, C, HW, per.data_ptr(), loss.data_ptr(), ops.stream())
    assert _last() == "hybrid_loss_fwd_kernel"
    L.lgm_hybrid_loss_bwd(*head, gl.data_ptr(), B, C, HW, gout.data_ptr(), ops.stream())
    assert _last() == "hybrid_loss_bwd_kernel"
    # the prediction lanes' twin: lgm_weighted_mse_bwd on operands of one pitch
    tg8 = torch.zeros((B, HW, pitch), device=dev)
    tg8[..., :C] = tgd[..., :C]
    out8 = outd.clone()
    out8[..., C:] = 0.0
    gmse = torch.full((B, HW, pitch), NAN, device=dev)
    L.lgm_weighted_mse_bwd(out8.data_ptr(), tg8.data_ptr(), pitch, td.data_ptr(), gdd.loss_weight.data_ptr(), gl.data_ptr(), B, C,
                           HW, pitch, gmse.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(gout[..., :C], gmse[..., :C]), "lanes [0, C) are what lgm_weighted_mse_bwd writes"
    assert float(gout[..., 2 * C:].abs().sum()) == 0.0 and torch.isfinite(gout).all(), "padding lanes get 0"
    # float64 from the same float32 operands and tables, the objective's own x0 prediction
    tab64, lw64 = tab.double(), gd.loss_weight.double().cpu()
    p64 = pred.double()
    x0p64 = {"pred_x0": p64, "pred_v": sa.double() * xt.double() - s1.double() * p64,
             "pred_noise": R.double() * xt.double() - Rm1.double() * p64}[objective]
    v64 = v.double().requires_grad_(True)
    term = learned_terms64(tab64, t, x0.double(), xt.double(), x0p64, v64)
    vb_b = term.flatten(1).mean(1) / LN2
    mse_b = ((p64 - target.double()) ** 2).flatten(1).mean(1) * lw64[t]
    want = mse_b.mean() + float(torch.tensor(W_VB, dtype=torch.float32)) * vb_b.mean()
    (want * float(gl)).backward()
    perh = per.double().cpu()
    for b in range(B):
        parity(f"{objective} C={C}: mse_b[{b}]", abs(perh[0, b] - mse_b[b]) / abs(mse_b[b]), RTOL)
        parity(f"{objective} C={C}: vb_b[{b}] (t = {int(t[b])})", abs(perh[1, b] - vb_b[b].detach()) / abs(vb_b[b].detach()), RTOL)
    parity(f"{objective} C={C}: loss", abs(float(loss) - float(want.detach())) / abs(float(want.detach())), RTOL)
    gv = gout[..., C:2 * C].double().cpu().permute(0, 2, 1)
    for b in range(B):
        assert float(v64.grad[b].abs().max()) > 0
        parity(f"{objective} C={C}: variance-lane gradient, sample {b} (t = {int(t[b])}), relative L2 against float64",
               rel(gv[b], v64.grad[b]), gvar_bound)
    # where the probability is floored the gradient is exactly 0, and the sweep reaches such elements
    z = (x0[0] - x0p[0]).abs() / sigma[0]
    inv = 1.0 / sigma[0].double()
    mean0 = tab64[0, 3] * x0p64[0] + tab64[0, 4] * xt[0].double()
    plus, minus = approx_cdf(inv * (x0[0] - mean0 + 1 / 255)), approx_cdf(inv * (x0[0] - mean0 - 1 / 255))
    prob = torch.where(x0[0] < -0.999, plus, torch.where(x0[0] > 0.999, 1.0 - minus, plus - minus))
    floored = prob < 1e-12
    assert bool(floored.any()) and bool((z[floored] > 5).all()) and bool((v64.grad[0][floored] == 0).all())
    assert bool((gv[0][floored] == 0).all()), "a floored probability has gradient 0"


# ----------------------------------------------------------------------------------------------------------------------
# (c) - (f): the small network of the fixture
# ----------------------------------------------------------------------------------------------------------------------
class _Case:
    def __init__(self, fx, dev):
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        from oracle import diffusion as OD
        self.fx, self.dev = fx, dev
        self.dim, self.S, self.B, self.T = int(fx["dim"]), int(fx["S"]), int(fx["B"]), int(fx["T"])
        self.P = OD.unet_init(dim=self.dim, channels=3, seed=int(fx["seed"]))
        self.P["final_conv.weight"] = torch.as_tensor(fx["final_conv.weight"])
        self.P["final_conv.bias"] = torch.as_tensor(fx["final_conv.bias"])
        self.net = Unet(dim=self.dim, channels=3, learned_variance=True)
        self.net.load_state_dict(self.P, strict=True)
        self.gd = GaussianDiffusion(self.net, img_size=self.S, timesteps=self.T, objective="pred_v", beta_schedule="cosine",
                                    vb_loss_weight=float(fx["vb_weight"])).to(dev)
        self.net.prepare_hip(dev)
        self.img, self.noise = torch.as_tensor(fx["img"]), torch.as_tensor(fx["noise"])
        self.t = torch.as_tensor(fx["times"])

    def plain(self):
        """a network without the head holding the prediction rows of final_conv, and its diffusion"""
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        P = dict(self.P)
        P["final_conv.weight"], P["final_conv.bias"] = P["final_conv.weight"][:3].clone(), P["final_conv.bias"][:3].clone()
        net = Unet(dim=self.dim, channels=3)
        net.load_state_dict(P, strict=True)
        return net, P


@pytest.fixture(scope="module")
def case(fx, dev):
    return _Case(fx, dev)


def test_training_step_matches_fixture(case, parity, gvar_bound):
    fx, gd, net, dev = case.fx, case.gd, case.net, case.dev
    from models.generative.diffusion import ddpm as D
    net._flat.zero_grad()
    loss, ctx = D.hip_loss_forward(gd, case.img.to(dev), case.t.to(dev), case.noise.to(dev), True, True)
    per, out = ctx.per.double().cpu(), ctx.out
    parity("unet_out, all 6 channels", rel(out[..., :6].permute(0, 3, 1, 2), fx["unet_out64"]), RTOL)
    parity("loss", abs(float(loss) - float(fx["loss64"])) / float(fx["loss64"]), RTOL)
    for b in range(case.B):
        parity(f"mse_b[{b}]", abs(per[0, b] - fx["mse_b64"][b]) / fx["mse_b64"][b], RTOL)
        parity(f"vb_b[{b}] (t = {int(case.t[b])})", abs(per[1, b] - fx["vb_b64"][b]) / fx["vb_b64"][b], RTOL)
    st = D.hip_loss_backward_begin(ctx, torch.ones(1, device=dev))
    gout = st.gout.clone()
    net.backward_run(st)
    torch.cuda.synchronize()
    g = gout[..., :6].permute(0, 3, 1, 2).double().cpu()
    want = torch.as_tensor(fx["gout64"])
    parity("output gradient, prediction lanes", rel(g[:, :3], want[:, :3]), RTOL)
    d = rel(g[:, 3:], want[:, 3:])
    parity.record("output gradient, variance lanes", device=d, float32_autograd=float(fx["gvar_dist"]))
    parity("output gradient, variance lanes: device against float64 (bound: twice float32 autograd's distance)", d, gvar_bound)
    for b in range(case.B):
        assert float(g[b, 3:].abs().max()) > 0, f"sample {b} has no variance-lane gradient"
        parity(f"output gradient, variance lanes of sample {b} (t = {int(case.t[b])})", rel(g[b, 3:], want[b, 3:]), gvar_bound)
    assert float(gout[..., 6:].abs().sum()) == 0.0
    # every parameter gradient: 1e-4 against float64, a miss decided by the float32 reference's own distance
    sd = dict(net.named_parameters())
    worst, n_seen = 0.0, 0
    for n, p in sd.items():
        flat = p.grad.reshape(-1).double().cpu()
        if "grad:" + n in fx:
            e = rel(flat, fx["grad:" + n].reshape(-1))
        else:
            ref = fx["gradsample:" + n]
            e = rel(flat[:: flat.numel() // ref.size][:ref.size], ref)
            en = abs(float(flat.norm()) - float(fx["gradnorm:" + n])) / float(fx["gradnorm:" + n])
            assert en < RTOL, (n, en)
        n_seen += 1
        worst = max(worst, e)
        if e >= RTOL:
            d_ref = float(fx["dref:" + n])
            parity.record(f"parameter gradient {n} [float64 arbiter]", hip_vs_fp64=e, ref_vs_fp64=d_ref)
            assert e <= 2 * d_ref, (n, e, d_ref)
    assert n_seen == len(case.P)
    parity.record("worst parameter gradient against float64", err=worst)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    parity("all-parameter gradient norm", abs(gn - float(fx["gradnorm_all"])) / float(fx["gradnorm_all"]), RTOL)
    # the public path gives the same loss bits
    again = gd.p_losses(case.img.to(dev), case.t.to(dev), case.noise.to(dev), _normalize=True)
    assert torch.equal(again.detach().reshape(1), loss)


def test_final_conv_of_the_64_channel_network_runs_the_narrow_kernels(dev, parity):
    """dim = 64: final_conv is the 64 -> 6 layer the Nw = 8 kernels were written for.  Forward and input gradient must note
    them; the weight and bias gradient (whichever kernel takes Nw = 8) against float64 from the saved operands, in the
    ledger's units for a reduction over B H W = 128 pixels."""
    from lgm_hip import ops
    from models.generative.diffusion import ddpm as D
    torch.manual_seed(3)
    net = D.Unet(dim=64, channels=3, learned_variance=True)
    gd = D.GaussianDiffusion(net, img_size=8, timesteps=8, beta_schedule="cosine").to(dev)
    net.prepare_hip(dev)
    g = torch.Generator().manual_seed(4)
    img, nz = torch.rand(2, 3, 8, 8, generator=g).to(dev), torch.randn(2, 3, 8, 8, generator=g).to(dev)
    xin = net.input_buffer(2, 8, 8, img)
    ops.nchw_to_nhwc(img, net.x_slice(xin, pad=True))
    t = torch.tensor([0, 5], device=dev)
    net.forward_nhwc(xin, t, False)
    assert _last() == "narrow1x1_fwd_kernel"
    net._flat.zero_grad()
    loss, ctx = D.hip_loss_forward(gd, img, t, nz, True, True)
    fin = ctx.tape.fin.clone()
    st = D.hip_loss_backward_begin(ctx, torch.ones(1, device=dev))
    gout = st.gout.clone()
    fc, fp = net.final_conv, net._flat
    gx = torch.empty_like(fin)
    ops.conv_yx(fc.geom(2, 8, 8), gout, fp.ptr(fc.weight), None, None, gx, fp.tptr(fc.weight))
    assert _last() == "narrow1x1_dgrad_kernel"
    net.backward_run(st)
    torch.cuda.synchronize()
    want = gout.reshape(-1, 8)[:, :6].double().cpu() @ fc.weight.detach().reshape(6, 64).double().cpu()
    parity("final_conv 64 -> 6 input gradient against float64", rel(gx.reshape(-1, 64), want), RTOL)
    gy, x = gout.reshape(-1, 8)[:, :6].double().cpu(), fin.reshape(-1, 64).double().cpu()
    e = bounds.forward_error_units(net.final_conv.weight.grad.reshape(6, 64), gy.T @ x, gy.abs().T @ x.abs())
    parity("final_conv 64 -> 6 weight gradient: worst element in units of 2^-24 S", e, bounds.tolerance(128))
    e = bounds.forward_error_units(net.final_conv.bias.grad, gy.sum(0), gy.abs().sum(0))
    parity("final_conv 64 -> 6 bias gradient: worst element in units of 2^-24 S", e, bounds.tolerance(128))
    assert torch.isfinite(loss).all()


def test_p_sample_and_vlb_terms_match_fixture(case, parity):
    fx, gd, dev = case.fx, case.gd, case.dev
    x, nz = torch.as_tensor(fx["ps:x"]).to(dev), torch.as_tensor(fx["ps:noise"]).to(dev)
    for ti in fx["ps_times"].tolist():
        got, x0 = gd.p_sample(x, ti, noise=nz)
        assert _last() == "sample_step_slice_kernel"
        parity(f"p_sample t = {ti}: x_(t-1)", rel(got, fx[f"ps:{ti}:out64"]), RTOL)
        parity(f"p_sample t = {ti}: x0", rel(x0, fx[f"ps:{ti}:x064"]), RTOL)
    img = torch.as_tensor(fx["img"])
    r = gd.vlb_terms(img, noise=list(torch.as_tensor(fx["vlb:noise"])), variance="learned")
    for i, ti in enumerate(r.timesteps):
        for b in range(case.B):
            e = abs(float(r.vb[i, b]) - fx["vlb:vb64"][i, b]) / abs(fx["vlb:vb64"][i, b])
            parity(f"vlb_terms learned, t = {ti}, sample {b}", e, RTOL)
    parity("vlb_terms learned: xstart_mse", rel(r.xstart_mse, fx["vlb:xstart_mse64"]), RTOL)
    parity("vlb_terms learned: mse", rel(r.mse, fx["vlb:mse64"]), RTOL)
    parity("vlb_terms learned: prior", rel(r.prior_bpd, fx["vlb:prior64"]), RTOL)
    parity("vlb_terms learned: total_bpd", rel(r.total_bpd, fx["vlb:total64"]), RTOL)
    small = gd.vlb_terms(img, noise=list(torch.as_tensor(fx["vlb:noise"])))
    assert rel(small.vb, fx["vlb:vb64"]) > 10 * RTOL, "the learned variance moves the bound by far more than the bound's tolerance"
    assert torch.equal(small.xstart_mse, r.xstart_mse)


def test_graph_replay_equals_eager_launches(case, dev, monkeypatch):
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import DDPM
    fx, gd = case.fx, case.gd
    shape = (case.B, 3, case.S, case.S)
    # the ancestral chain under injected draws
    g = torch.Generator().manual_seed(31)
    init = torch.randn(shape, generator=g).to(dev)
    noises = [torch.randn(shape, generator=g).to(dev) for _ in range(case.T)]
    key = sampler._graph_key(gd, shape, True, False, False, False, learned=True)
    assert key[0] == "learned" and key not in {sampler._graph_key(gd, shape, True, False, False, False)}
    graph = sampler.p_sample_loop(gd, shape, init_noise=init, noises=noises)
    assert isinstance(sampler._GRAPHS[case.net].get(key), sampler._GraphedChain), "the learned chain was captured under its key"
    vg = gd.vlb_terms(torch.as_tensor(fx["img"]), noise=list(torch.as_tensor(fx["vlb:noise"])), variance="learned")
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = sampler.p_sample_loop(gd, shape, init_noise=init, noises=noises)
    ve = gd.vlb_terms(torch.as_tensor(fx["img"]), noise=list(torch.as_tensor(fx["vlb:noise"])), variance="learned")
    monkeypatch.delenv("LGM_NO_SAMPLER_GRAPH")
    assert torch.isfinite(graph).all() and torch.equal(graph, eager), "ancestral chain: graph replay and eager launches differ"
    for a, b in zip(vg[:5], ve[:5]):
        assert torch.equal(a, b), "likelihood loop: graph replay and eager launches differ"
    # one DDPMFastStep step
    def module():
        torch.manual_seed(10)
        m = DDPM(img_size=case.S, dim=case.dim, lr=1e-3, diffusion_timesteps=case.T, beta_schedule="cosine",
                 learned_variance=True, vb_loss_weight=0.01)
        m.sample_every = 0
        m.to(dev)
        m.prepare_hip(dev)
        m.train()
        return m
    a, b = module(), module()
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True), b.make_fast_step(ob, 1, False)
    x = torch.as_tensor(fx["img"]).to(dev)
    before = a.ema.online_model.model._flat.data.clone()
    losses = []
    for fast in (fa, fb):
        torch.manual_seed(77)
        losses.append(fast.step((x.clone(), None), 0).detach().clone().reshape(()))
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1]), (float(losses[0]), float(losses[1]))
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data), "parameters after the step: graph replay and eager launches differ"
    assert not torch.equal(na._flat.data, before)


def test_ddim_and_dpm_read_the_prediction_lanes_alone(case, dev):
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    shape = (case.B, 3, case.S, case.S)
    g = torch.Generator().manual_seed(41)
    init = torch.randn(shape, generator=g).to(dev)
    plain_net, _ = case.plain()
    for kw in (dict(sampling_timesteps=4), dict(sampling_timesteps=4, sampler="dpm++")):
        common = dict(img_size=case.S, timesteps=case.T, objective="pred_v", beta_schedule="cosine", **kw)
        lg = GaussianDiffusion(case.net, **common).to(dev)
        pg = GaussianDiffusion(plain_net, **common).to(dev)
        plain_net.prepare_hip(dev)
        fn = sampler.dpm_solver_sample if "sampler" in kw else sampler.ddim_sample
        a, b = fn(lg, shape, init_noise=init), fn(pg, shape, init_noise=init)
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{kw}: the chain read more than the prediction lanes"
        t = torch.full((case.B,), 3, device=dev, dtype=torch.long)
        pa, pb = lg.model_predictions(init, t, clip_x_start=True), pg.model_predictions(init, t, clip_x_start=True)
        assert torch.equal(pa.pred_x_start, pb.pred_x_start) and torch.equal(pa.pred_noise, pb.pred_noise)
    # guidance mixes the prediction lanes; the variance lanes stay the conditional forward's
    torch.manual_seed(5)
    net = Unet(dim=case.dim, channels=3, learned_variance=True, num_classes=4)
    cg = GaussianDiffusion(net, img_size=case.S, timesteps=case.T, beta_schedule="cosine").to(dev)
    net.prepare_hip(dev)
    x = net.input_buffer(case.B, case.S, case.S, init)
    from lgm_hip import ops
    ops.nchw_to_nhwc(init.contiguous(), net.x_slice(x, pad=True))
    t = torch.full((case.B,), 5, device=dev, dtype=torch.long)
    y = net.labels(torch.tensor([0, 1, 2, 3]), case.B, dev)
    cond = net.forward_guided(x, t, y, 1.0).clone()
    null = net.forward_guided(x, t, None, 1.0).clone()
    mix = net.forward_guided(x, t, y, 3.0).clone()
    assert torch.equal(mix[..., 3:6], cond[..., 3:6]) and not torch.equal(cond[..., 3:6], null[..., 3:6])
    assert not torch.equal(mix[..., :3], cond[..., :3])
    assert cg.learned_variance
