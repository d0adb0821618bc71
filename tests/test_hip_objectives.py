"""GPU: GaussianDiffusion on the pred_noise (eps) and pred_x0 objectives, with offset noise.

  * the four ``lgm_*_obj`` entry points against float64 restatements, objective 2 (pred_v) bit for bit against the plain
    entry points, and the kernel each of them launches;
  * training step, model_predictions and sampling against what the REFERENCE's GaussianDiffusion returned for both
    objectives (tests/golden/diffusion_objectives.npz, written by tools/make_golden_objectives.py), 1e-4 relative;
  * the timed paths (graph-replayed training step, graph-replayed sampler) bit for bit against eager launches;
  * train.py on configs/diffusion/ddpm_eps.json.

Where a sampling loop or an unclipped x_start misses 1e-4 against the reference's fp32 result the float64 arbiter of
DESIGN section 1.1 decides (``_Arbiter``): HIP must be no further from float64 than twice the reference itself is; every
other quantity has to meet 1e-4.  Every measured distance goes through the ``parity`` recorder (LGM_PARITY_LOG; the committed record is profiles/r07_objectives_parity.json).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24                        # unit roundoff of float32


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)      # Downsample's weight: held as [N, C, 2, 2], row-major = the reference's [N, 4 C, 1, 1]
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_objectives.npz")))


@pytest.fixture(scope="module")
def tables():
    """The product's fp32 schedule tables (host copies)."""
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)
    return {n: getattr(gd, n).clone() for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                                "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")}


# ----------------------------------------------------------------------------------------------------------------------
# kernels.  B = 3, 5 x 7 pixels, C = 3 / 1 in 4 padded channels: padded channels, a pixel count that is no power of two and
# a partial last block (420 threads of work for 256-thread blocks); t = 0 / 517 / 999: both ends of the tables.
# A float32 result is compared with the float64 value element by element against 8 u M.  Every rounding is at most
# u = 2^-24 relative to its own partial result and M is the sum of the magnitudes of the terms of the expression (a
# difference divided by Rm1 carries its terms' magnitudes divided by Rm1), so to first order: x_start <= 2 u M (two
# products, one difference), pred_noise <= 2 u M on top of x_start's share, x_t and v <= 3 u M (the offset sum and the
# normalisation feed two products and a sum), the sampler update <= 6 u M (x0 and eps as above, four products, three sums).
# ----------------------------------------------------------------------------------------------------------------------
KB, KH, KW, KCP = 3, 5, 7, 4
KT = (0, 517, 999)


def _within(got, want, bound, what):
    got, want = got.detach().double().cpu(), want.double()
    excess = ((got - want).abs() - 8 * U * bound.double()).max().item()
    assert excess <= 0, f"{what}: error exceeds 8 u M by {excess:.3e}"
    return float(((got - want).abs() / bound.double().clamp_min(1e-300)).max() / U)


def _last(L):
    return L._dll.lgm_last_kernel().decode()


def _nhwc(x, C):
    """[B, H W, Cpad] device tensor -> (NCHW host view of the C real channels, the padded channels)"""
    x = x.cpu().reshape(KB, KH, KW, KCP)
    return x[..., :C].permute(0, 3, 1, 2), x[..., C:]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("with_offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("objective", [0, 1, 2], ids=["pred_noise", "pred_x0", "pred_v"])
def test_qsample_target_obj_kernel(dev, tables, objective, with_offset, C):
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
    xt = torch.full((KB, KH * KW, KCP), 7.0, device=dev)
    tg = torch.full((KB, KH * KW, KCP), 7.0, device=dev)
    L.lgm_qsample_target_obj(imgd.data_ptr(), noised.data_ptr(), offd.data_ptr() if with_offset else None, strength,
                             td.data_ptr(), sad.data_ptr(), sbd.data_ptr(), 1, objective, xt.data_ptr(), tg.data_ptr(),
                             KCP, KB, C, KH * KW, KCP, ops.stream())
    assert _last(L) == "qsample_slice_kernel"
    torch.cuda.synchronize()
    assert torch.equal(noised.cpu(), noise), "the kernel must not write the caller's noise"
    # float64 restatement (reference ddpm.py:889-891, 869-876, 911-917) of the float32 inputs
    s32 = float(torch.tensor(strength, dtype=torch.float32))
    a, b = sa[t].double()[:, None, None, None], sb[t].double()[:, None, None, None]
    x0 = img.double() * 2 - 1
    shift = s32 * off.double()[:, :, None, None] if with_offset else torch.zeros(KB, C, 1, 1, dtype=torch.float64)
    n = noise.double() + shift
    n_mag = noise.double().abs() + shift.abs()
    want_xt, m_xt = a * x0 + b * n, a * (2 * img.double() + 1) + b * n_mag
    want_tg, m_tg = [(n, n_mag), (x0, 2 * img.double() + 1),
                     (a * n - b * x0, a * n_mag + b * (2 * img.double() + 1))][objective]
    got_xt, pad_xt = _nhwc(xt, C)
    got_tg, pad_tg = _nhwc(tg, C)
    _within(got_xt, want_xt, m_xt, "x_t")
    _within(got_tg, want_tg, m_tg, "target")
    assert float(pad_xt.abs().max()) == 0 and float(pad_tg.abs().max()) == 0, "padded channels are written as zero"
    if objective == 1:
        assert torch.equal(got_tg, img * 2 - 1)
    if objective == 0 and not with_offset:
        assert torch.equal(got_tg, noise)
    if objective == 2 and not with_offset:                     # the bits of the plain entry point
        xt2, tg2 = torch.full_like(xt, 7.0), torch.full_like(tg, 7.0)
        L.lgm_qsample_target(imgd.data_ptr(), noised.data_ptr(), td.data_ptr(), sad.data_ptr(), sbd.data_ptr(), 1,
                             xt2.data_ptr(), tg2.data_ptr(), KCP, KB, C, KH * KW, KCP, ops.stream())
        assert _last(L) == "qsample_slice_kernel"
        assert torch.equal(xt, xt2) and torch.equal(tg, tg2)


def _predictions64(objective, x, out, t, tb, clip, rederive):
    """reference ddpm.py:707-734 in float64 -> (pred_noise, its bound M, x_start, its bound M)"""
    ex = lambda n: tb[n][t].double()[:, None, None, None]  # noqa: E731
    A, S, R, Rm1 = (ex(n) for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                    "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"))
    x, out = x.double(), out.double()
    if objective == 0:
        x0, m0 = R * x - Rm1 * out, (R * x).abs() + (Rm1 * out).abs()
    elif objective == 1:
        x0, m0 = out, out.abs()
    else:
        x0, m0 = A * x - S * out, (A * x).abs() + (S * out).abs()
    if clip:
        x0 = x0.clamp(-1.0, 1.0)                               # 1-Lipschitz: the bound carries over
    if objective == 0 and not (clip and rederive):
        return out, out.abs(), x0, m0
    pn = (R * x - x0) / Rm1
    return pn, ((R * x).abs() + x0.abs() + m0) / Rm1 + pn.abs(), x0, m0


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("clip,rederive", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("objective", [0, 1, 2], ids=["pred_noise", "pred_x0", "pred_v"])
def test_model_predictions_obj_kernel(dev, tables, objective, clip, rederive, C):
    from lgm_hip import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(50 + C)
    x = torch.randn(KB, C, KH, KW, generator=g)
    out = torch.randn(KB, C, KH, KW, generator=g)
    t = torch.tensor(KT)
    d = lambda v: v.to(dev).contiguous()  # noqa: E731
    xd, outd, td = d(x), d(out), d(t)
    tbd = [d(tables[n]) for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                                  "sqrt_recipm1_alphas_cumprod")]
    pn, xs = torch.empty_like(xd), torch.empty_like(xd)
    L.lgm_model_predictions_obj(xd.data_ptr(), outd.data_ptr(), td.data_ptr(), *[b.data_ptr() for b in tbd], objective,
                                clip, rederive, pn.data_ptr(), xs.data_ptr(), KB, C * KH * KW, 1000, ops.stream())
    want_pn, m_pn, want_xs, m_xs = _predictions64(objective, x, out, t, tables, clip, rederive)
    _within(xs, want_xs, m_xs, "x_start")
    _within(pn, want_pn, m_pn, "pred_noise")
    if clip:
        assert float(xs.abs().max()) <= 1.0
    if objective == 0 and not (clip and rederive):
        assert torch.equal(pn.cpu(), out), "pred_noise stays the raw network output (reference :716, 720)"
    if objective == 1 and not clip:
        assert torch.equal(xs.cpu(), out)
    if objective == 2:                                         # rederive has no effect; the bits of lgm_model_predictions
        pn2, xs2 = torch.empty_like(xd), torch.empty_like(xd)
        L.lgm_model_predictions(xd.data_ptr(), outd.data_ptr(), td.data_ptr(), *[b.data_ptr() for b in tbd], clip,
                                pn2.data_ptr(), xs2.data_ptr(), KB, C * KH * KW, 1000, ops.stream())
        assert torch.equal(pn, pn2) and torch.equal(xs, xs2)


@pytest.mark.parametrize("C", [3, 1])
def test_sample_step_obj_kernels(dev, tables, C):
    """lgm_sample_step_obj: objective 2 gives lgm_sample_step's bits; for every objective (x0, eps) are those of
    lgm_model_predictions_obj at the shared timestep and the update is C0 x0 + C1 x + C2 eps + C3 noise; the table-driven
    in-place form gives the by-value form's bits (row 1 of a two-row table)."""
    from lgm_hip import ops
    L = ops.lib()
    g = torch.Generator().manual_seed(60 + C)
    HW = KH * KW
    x = torch.zeros(KB, HW, KCP)
    v = torch.zeros(KB, HW, KCP)
    x[..., :C] = torch.randn(KB, HW, C, generator=g)
    v[..., :C] = torch.randn(KB, HW, C, generator=g)
    v[..., C:] = 3.0                                           # a padded lane of the network output is never used
    nz = torch.randn(KB, C, KH, KW, generator=g)
    tq = 517
    A, Bv = float(tables["sqrt_alphas_cumprod"][tq]), -float(tables["sqrt_one_minus_alphas_cumprod"][tq])
    R, Rm1 = float(tables["sqrt_recip_alphas_cumprod"][tq]), float(tables["sqrt_recipm1_alphas_cumprod"][tq])
    C0, C1, C2, C3 = 0.75, 0.125, 0.5, 0.25
    xd, vd, nzd = x.to(dev), v.to(dev), nz.to(dev)
    table = torch.tensor([[0.0] * 8, [A, Bv, R, Rm1, C0, C1, C2, C3]], device=dev)
    counter = torch.ones(1, dtype=torch.int32, device=dev)
    tb = {k: b[tq:tq + 1].expand(KB).contiguous() for k, b in tables.items()}     # per-sample tables at the shared t
    tzero = torch.zeros(KB, dtype=torch.long)
    for objective in (0, 1, 2):
        for clip, red in ((1, 0), (1, 1), (0, 0)):
            o, x0 = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
            L.lgm_sample_step_obj(xd.data_ptr(), vd.data_ptr(), nzd.data_ptr(), o.data_ptr(), x0.data_ptr(), KB, C, HW,
                                  KCP, objective, A, Bv, clip, red, R, Rm1, C0, C1, C2, C3, ops.stream())
            assert _last(L) == "sample_step_slice_kernel"
            xi = xd.clone()
            x0i = torch.full_like(xd, 7.0)
            L.lgm_sample_step_table_obj(xi.data_ptr(), vd.data_ptr(), nzd.data_ptr(), x0i.data_ptr(), KB, C, HW, KCP,
                                        table.data_ptr(), counter.data_ptr(), objective, clip, red, 0, ops.stream())
            assert _last(L) == "sample_step_slice_kernel"
            assert torch.equal(xi, o) and torch.equal(x0i, x0), (objective, clip, red)
            assert int(counter) == 1
            got_o, pad_o = _nhwc(o, C)
            got_x0, pad_x0 = _nhwc(x0, C)
            assert float(pad_o.abs().max()) == 0 and float(pad_x0.abs().max()) == 0
            xn, vn = _nhwc(xd, C)[0], _nhwc(vd, C)[0]
            pn, m_pn, xs, m_xs = _predictions64(objective, xn, vn, tzero, tb, clip, red)
            _within(got_x0, xs, m_xs, "x0")
            want = C0 * xs + C1 * xn.double() + C2 * pn + C3 * nz.double()
            _within(got_o, want, C0 * m_xs + C1 * xn.double().abs() + C2 * m_pn + C3 * nz.double().abs(), "update")
            if objective == 2:
                o2, x02 = torch.empty_like(xd), torch.empty_like(xd)
                L.lgm_sample_step(xd.data_ptr(), vd.data_ptr(), nzd.data_ptr(), o2.data_ptr(), x02.data_ptr(), KB, C, HW,
                                  KCP, A, Bv, clip, R, Rm1, C0, C1, C2, C3, ops.stream())
                assert _last(L) == "sample_step_slice_kernel"
                assert torch.equal(o, o2) and torch.equal(x0, x02)
    xi = xd.clone()
    L.lgm_sample_step_table_obj(xi.data_ptr(), vd.data_ptr(), None, None, KB, C, HW, KCP, table.data_ptr(),
                                counter.data_ptr(), 0, 1, 0, 1, ops.stream())
    assert _last(L) == "sample_step_slice_kernel"
    assert int(counter) == 2                                   # advance != 0 appends counter += 1


# ----------------------------------------------------------------------------------------------------------------------
# parity with the reference's GaussianDiffusion for both new objectives (dim 16, 16 x 16, B = 2, t = (37, 912))
# ----------------------------------------------------------------------------------------------------------------------
class _Case:
    def __init__(self, fx, objective, dev):
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        from oracle import diffusion as OD
        self.o, self.dev = objective, dev
        self.dim, self.S, self.B = int(fx["dim"]), int(fx["S"]), int(fx["B"])
        self.P = OD.unet_init(dim=self.dim, channels=3, seed=int(fx["seed"]))
        g = torch.Generator().manual_seed(int(fx["data_seed"]))
        self.img = torch.rand(self.B, 3, self.S, self.S, generator=g)
        self.noise = torch.randn(self.B, 3, self.S, self.S, generator=g)
        self.t = torch.as_tensor(fx["t"])
        self.net = Unet(dim=self.dim, channels=3)
        self.net.load_state_dict(self.P, strict=True)
        self.gd = GaussianDiffusion(self.net, img_size=self.S, timesteps=1000, sampling_timesteps=50,
                                    objective=objective).to(dev)
        self.net.prepare_hip(dev)
        self.fx = {k[len(objective) + 1:]: v for k, v in fx.items() if k.startswith(objective + ":")}
        self.x_t = torch.as_tensor(self.fx["x_t"])


@pytest.fixture(scope="module", params=["pred_noise", "pred_x0"])
def case(request, fx, dev):
    return _Case(fx, request.param, dev)


class _Arbiter:
    """the same quantity on the CPU in float64 (oracle.diffusion.unet_forward on .double() parameters
    plus the reference's algebra :673-757, 805-829 on the float32 tables).  ``check``: 1e-4 against the reference's fp32
    result; with ``exact_fn`` (the sampling loops and the unclipped x_start only: at t = 999 x0 = R x - Rm1 eps has
    R = 1.8e3) a miss is decided by float64 - HIP no further from it than 2 x the reference's own distance (the factor 2
    covers the different summation order of two fp32 evaluations).  All distances are recorded."""

    def __init__(self, case):
        from oracle import diffusion as OD
        self.c, self.OD = case, OD
        self.P64 = {k: v.double() for k, v in case.P.items()}
        self.bufs = {}

    def tab(self, T):
        if T not in self.bufs:
            self.bufs[T] = {k: v.double() for k, v in self.OD.diffusion_buffers(T).items()}
        return self.bufs[T]

    def predictions(self, x, t, clip, rederive, T=1000):
        b, o = self.tab(T), self.c.o
        ex = lambda n: b[n][t][:, None, None, None]  # noqa: E731
        x = x.double()
        with torch.no_grad():
            out = self.OD.unet_forward(self.P64, x, t.double(), self.c.dim)
        R, Rm1 = ex("sqrt_recip_alphas_cumprod"), ex("sqrt_recipm1_alphas_cumprod")
        x0 = R * x - Rm1 * out if o == "pred_noise" else out
        if clip:
            x0 = x0.clamp(-1.0, 1.0)
        if o == "pred_noise" and not (clip and rederive):
            return out, x0
        return (R * x - x0) / Rm1, x0

    def p_sample(self, x, ti, noise, T=1000):
        b = self.tab(T)
        t = torch.full((x.shape[0],), ti, dtype=torch.long)
        _, x0 = self.predictions(x, t, True, False, T)
        mean = b["posterior_mean_coef1"][ti] * x0 + b["posterior_mean_coef2"][ti] * x.double()
        return mean + (0.5 * b["posterior_log_variance_clipped"][ti]).exp() * noise.double() if ti > 0 else mean

    def ddim(self, x, ti, tn, T=1000):
        b = self.tab(T)
        pn, x0 = self.predictions(x, torch.full((x.shape[0],), ti, dtype=torch.long), True, True, T)
        if tn < 0:
            return x0
        an = b["alphas_cumprod"][tn]
        return x0 * an.sqrt() + (1 - an).sqrt() * pn            # eta = 0

    def ddim_loop(self, init, pairs):
        x = init.double()
        for ti, tn in pairs:
            x = self.ddim(x, ti, tn)
        return (x + 1) * 0.5

    def p_sample_loop(self, init, noises, T):
        x = init.double()
        for i, ti in enumerate(reversed(range(T))):
            x = self.p_sample(x, ti, noises[i] if ti > 0 else None, T)
        return (x + 1) * 0.5

    def check(self, parity, what, hip, ref, exact_fn=None):
        what = f"{self.c.o}: {what}"
        e = rel(hip, ref)
        if e < RTOL or exact_fn is None:
            return parity(what, e, RTOL)
        exact = exact_fn()
        d_ref, d_hip = rel(ref, exact), rel(hip, exact)
        parity.record(what + " [float64 arbiter]", hip_vs_ref=e, ref_vs_fp64=d_ref, hip_vs_fp64=d_hip)
        print(f"[parity] {what}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, "
              f"hip {d_hip:.3e}")
        assert d_hip <= 2 * d_ref, (what, e, d_hip, d_ref)


@pytest.fixture(scope="module")
def arbiter(case):
    return _Arbiter(case)


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
    parity(f"{case.o}{tag}: worst parameter gradient (23 whole tensors)", worst, RTOL)
    parity(f"{case.o}{tag}: worst gradient norm (3 large tensors)", worst_n, RTOL)
    parity(f"{case.o}{tag}: worst 1024-element gradient sample (3 large tensors)", worst_s, RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    want = float(fx[pre + "gradnorm_all"])
    parity(f"{case.o}{tag}: all-parameter gradient norm", abs(gn - want) / want, RTOL)


def test_training_step_matches_reference_fixture(case, parity):
    fx, gd, net, dev = case.fx, case.gd, case.net, case.dev
    x0 = (case.img * 2 - 1).to(dev)
    parity(f"{case.o}: q_sample vs the reference's x_t", rel(gd.q_sample(x0, case.t.to(dev), case.noise.to(dev)), fx["x_t"]),
           1e-6)
    with torch.no_grad():
        out = net(case.x_t.to(dev), case.t.to(dev))
    parity(f"{case.o}: unet_out", rel(out, fx["unet_out"]), RTOL)
    net._flat.zero_grad()
    loss = gd.p_losses(x0, case.t.to(dev), case.noise.to(dev))
    parity(f"{case.o}: loss", abs(loss.item() - float(fx["loss"])) / float(fx["loss"]), RTOL)
    loss.backward()
    _grad_checks(parity, case, "", "")


def test_offset_noise_training_step_matches_reference_fixture(case, fx, parity):
    cfx, gd, net, dev = case.fx, case.gd, case.net, case.dev
    x0 = (case.img * 2 - 1).to(dev)
    noise = case.noise.to(dev)
    off = torch.as_tensor(cfx["offset_noise"]).to(dev)
    strength = float(fx["offset_strength"])
    with torch.no_grad():
        out = net(torch.as_tensor(cfx["offset:x_t"]).to(dev), case.t.to(dev))
    parity(f"{case.o}, offset noise: unet_out", rel(out, cfx["offset:unet_out"]), RTOL)
    net._flat.zero_grad()
    loss = gd.p_losses(x0, case.t.to(dev), noise, offset_noise_strength=strength, _offset_noise=off)
    assert torch.equal(noise.cpu(), case.noise), "p_losses must not write the caller's noise"
    want = float(cfx["offset:loss"])
    parity(f"{case.o}, offset noise: loss", abs(loss.item() - want) / want, RTOL)
    assert abs(want - float(cfx["loss"])) / want > RTOL, "the offset moves the reference's loss by more than the bound"
    loss.backward()
    _grad_checks(parity, case, "offset:", ", offset noise")
    # the instance's strength is the default, an explicit 0 switches it off, and without an injected draw the [B, C]
    # offsets come from the device generator
    gd.offset_noise_strength = strength
    try:
        with torch.no_grad():
            again = gd.p_losses(x0, case.t.to(dev), noise, _offset_noise=off)
            plain = gd.p_losses(x0, case.t.to(dev), noise, offset_noise_strength=0.0)
            torch.manual_seed(5)
            drawn = gd.p_losses(x0, case.t.to(dev), noise)
            torch.manual_seed(5)
            drawn2 = gd.p_losses(x0, case.t.to(dev), noise, _offset_noise=torch.randn(2, 3, device=dev))
    finally:
        gd.offset_noise_strength = 0.0
    assert abs(again.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert abs(plain.item() - float(cfx["loss"])) / float(cfx["loss"]) < RTOL
    assert torch.equal(drawn, drawn2) and not torch.equal(drawn, again)


@pytest.mark.parametrize("clip,rederive", [(False, False), (False, True), (True, False), (True, True)])
def test_model_predictions_match_reference_fixture(case, arbiter, parity, clip, rederive):
    dev = case.dev
    pred = case.gd.model_predictions(case.x_t.to(dev), case.t.to(dev), clip_x_start=clip, rederive_pred_noise=rederive)
    assert type(pred).__name__ == "ModelPrediction"
    key = f"mp:{int(clip)}{int(rederive)}:"
    arbiter.check(parity, f"pred_noise, clip={clip} rederive={rederive}", pred.pred_noise, case.fx[key + "pred_noise"])
    arbiter.check(parity, f"pred_x_start, clip={clip} rederive={rederive}", pred.pred_x_start, case.fx[key + "x_start"],
                  None if clip else (lambda: arbiter.predictions(case.x_t, case.t, clip, rederive)[1]))
    if clip:                                                   # p_mean_variance (:736-746) clips the same x_start
        mean, _, _, xs = case.gd.p_mean_variance(case.x_t.to(dev), case.t.to(dev), clip_denoised=True)
        assert torch.equal(xs, pred.pred_x_start) and torch.isfinite(mean).all()


def test_sampling_steps_match_reference_fixture(case, arbiter, parity):
    from lgm_hip import sampler
    fx, gd, dev = case.fx, case.gd, case.dev
    shape = tuple(case.x_t.shape)
    nz = torch.as_tensor(fx["p_sample_noise"])
    ch = sampler._Chain(gd, shape, case.x_t.to(dev))
    sampler.p_sample_step(ch, 500, nz.to(dev))
    arbiter.check(parity, "p_sample t=500", ch.image(False), fx["p_sample_500"])
    img, x0 = gd.p_sample(case.x_t.to(dev), 500, noise=nz.to(dev))     # the public method takes the same route
    assert torch.equal(img, ch.image(False)) and float(x0.abs().max()) <= 1.0
    ch = sampler._Chain(gd, shape, case.x_t.to(dev))
    sampler.p_sample_step(ch, 0, None)
    arbiter.check(parity, "p_sample t=0", ch.image(False), fx["p_sample_0"])
    ch = sampler._Chain(gd, shape, case.x_t.to(dev))
    sampler.ddim_step(ch, 999, 979, None, 0.0)
    arbiter.check(parity, "ddim 999->979", ch.image(False), fx["ddim_999_979"])


def test_whole_sampling_loops_match_reference_fixture(case, fx, arbiter, parity):
    """The reference's complete loops for the objective, replaying its CPU-generator draws (as tests/test_hip_unet.py does
    for pred_v): the 50-pair DDIM chain (eta = 0) and the 200-step ancestral chain."""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion
    from oracle import diffusion as OD
    gd, dev = case.gd, case.dev
    shape = tuple(case.x_t.shape)
    init, nz = OD.draw_loop_noise(int(fx["ddim_loop_seed"]), shape, 49)
    out = sampler.ddim_sample(gd, shape, init_noise=init.to(dev), noises=[n.to(dev) for n in nz] + [None])
    arbiter.check(parity, "50-pair DDIM loop, final image", out, case.fx["ddim_loop_50"],
                  lambda: arbiter.ddim_loop(init, gd.ddim_time_pairs()))
    gd_a = GaussianDiffusion(case.net, img_size=case.S, timesteps=200, objective=case.o).to(dev)
    init, nz = OD.draw_loop_noise(int(fx["p_sample_loop_seed"]), shape, 199)
    out = sampler.p_sample_loop(gd_a, shape, init_noise=init.to(dev), noises=[n.to(dev) for n in nz] + [None])
    arbiter.check(parity, "200-step ancestral loop, final image", out, case.fx["p_sample_loop_200"],
                  lambda: arbiter.p_sample_loop(init, nz + [None], 200))


# ----------------------------------------------------------------------------------------------------------------------
# the timed paths: graph replay against eager launches, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
TIMED = [dict(objective="pred_noise", offset_noise_strength=0.1, min_snr_loss_weight=True), dict(objective="pred_x0")]
TIMED_IDS = ["pred_noise_offset_minsnr", "pred_x0"]


def _module(dev, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(img_size=16, dim=16, lr=1e-3, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("kw", TIMED, ids=TIMED_IDS)
def test_graph_replayed_training_step_equals_eager_steps(dev, kw):
    """Three steps through ``make_fast_step(use_graph=True)`` (t, noise and the [B, C] offset noise drawn inside the
    captured graph) leave the parameters, Adam state and losses of three eager steps from the same seed."""
    a, b = _module(dev, **kw), _module(dev, **kw)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True), b.make_fast_step(ob, 1, False)
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(4, 3, 16, 16, generator=g).to(dev) for _ in range(3)]
    losses = {}
    for name, fast in (("graph", fa), ("eager", fb)):
        torch.manual_seed(77)                                  # the device generator: same draws in both runs
        losses[name] = [fast.step((x.clone(), None), i).detach().clone().reshape(()) for i, x in enumerate(xs)]
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    if kw.get("offset_noise_strength"):
        off = fa.graphed.offset
        assert off is not None and off.shape == (4, 3) and float(off.abs().max()) > 0
    else:
        assert fa.graphed.offset is None
    for la, lb in zip(losses["graph"], losses["eager"]):
        assert torch.isfinite(la) and torch.equal(la, lb), (float(la), float(lb))
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    for pa, pb in zip(oa.state_dict()["state"].values(), ob.state_dict()["state"].values()):
        for k in pb:
            assert torch.equal(torch.as_tensor(pa[k]), torch.as_tensor(pb[k])), k


@pytest.mark.parametrize("kw", TIMED, ids=TIMED_IDS)
def test_graph_replayed_sampling_equals_eager_chain(dev, kw, monkeypatch):
    """``sample(batch_size=2)`` by graph replay against the eager chain (LGM_NO_SAMPLER_GRAPH=1): the 5-pair DDIM chain
    (clip + re-derived noise) and a 6-step ancestral chain (clip only) with injected noise."""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion
    from oracle import diffusion as OD
    m = _module(dev, sampling_timesteps=5, **kw)
    gd = m.ema.ema_model
    gd.eval()
    assert gd.is_ddim_sampling and gd.objective == kw["objective"]
    gd_a = GaussianDiffusion(gd.model, img_size=16, timesteps=6, objective=kw["objective"]).to(dev)
    shape = (2, 3, 16, 16)
    init, nz = OD.draw_loop_noise(7, shape, 5)
    nzd = [n.to(dev) for n in nz] + [None]
    outs = {}
    for mode in ("graph", "eager"):
        monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0" if mode == "graph" else "1")
        torch.manual_seed(123)                                 # sample() draws its start image on the device
        outs[mode] = (gd.sample(batch_size=2).clone(),
                      sampler.p_sample_loop(gd_a, shape, init_noise=init.to(dev), noises=nzd).clone())
    per = sampler._GRAPHS[gd.model]
    assert set(per) == {(shape, False, kw["objective"], True), (shape, True, kw["objective"], False)}
    assert all(isinstance(e, sampler._GraphedChain) for e in per.values()), "graph capture did not happen"
    for ga, ea in zip(outs["graph"], outs["eager"]):
        assert ga.shape == shape and torch.isfinite(ga).all() and float(ga.std()) > 0
        assert torch.equal(ga, ea)
    # interpolate (:847-867) walks the same ancestral chain
    x1, x2 = torch.rand(2, 3, 16, 16, device=dev) * 2 - 1, torch.rand(2, 3, 16, 16, device=dev) * 2 - 1
    assert torch.isfinite(gd_a.interpolate(x1, x2, t=4)).all()


def test_train_entry_runs_the_eps_config(tmp_path):
    """python train.py --config_path configs/diffusion/ddpm_eps.json --max_steps 6 (pred_noise, min-SNR weights, offset
    noise 0.1; the step-0 sample is the 1000-step ancestral chain of the objective), then a resume."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = os.path.join(pkg, "configs", "diffusion", "ddpm_eps.json")
    exp = "pytest_gpu_diffusion_ddpm_eps"
    cmd = [sys.executable, os.path.join(pkg, "train.py"), "--config_path", cfg, "--max_steps", "6", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    name = json.load(open(cfg))["model"]["name"]
    ck = os.path.join(pkg, "experiments", name, exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 6 and len(sd["optimizer_states"]) >= 1
    hp = sd["hyper_parameters"]
    assert hp["objective"] == "pred_noise" and hp["offset_noise_strength"] == 0.1 and hp["min_snr_loss_weight"] is True
    for v in sd["state_dict"].values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
    r = subprocess.run(cmd[:-4] + ["--max_steps", "9", "--experiment_name", exp, "--ckpt_path", ck], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 9 and sd["hyper_parameters"]["objective"] == "pred_noise"
