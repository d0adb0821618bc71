"""GPU: low-resolution conditioning of a cascaded super-resolution stage (``Unet(lowres_cond=True)``; an extension of the
reference).

  * ``lgm_lowres_cond`` against the float64 restatement of tests/lowres_ref.py, per element, both sources, sentinel lanes, the
    unaugmented value and the agreement of the two sources bit for bit; the row-local embedding add against float64;
  * the conditioning slice after 6-step DDIM, ancestral and DPM-Solver++ chains, thresholded and not, eager and replayed;
  * network output, loss and ALL parameter gradients, a 20-pair DDIM chain, a 50-step ancestral chain and a guided
    class-conditional case against what the REFERENCE's modules returned as a self-conditioned network fed the conditioning
    image (tests/golden/diffusion_lowres.npz, tools/make_golden_lowres.py), 1e-4 relative or the float64 arbiter rule of
    tests/test_hip_objectives.py;
  * graph replay bit for bit against eager launches (training step, also accumulating with dropout; every sampler), fresh
    draws of s and eps per replay, and a plain model's random stream untouched; train.py on configs/diffusion/ddpm_sr_32_128.json.

Measured distances go through the ``parity`` recorder (committed record: profiles/r18_lowres_parity.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lowres_ref as LR

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = LR.U
SENTINEL = 7.0


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_lowres.npz")))


def _tables(T=1000):
    from models.generative.diffusion.ddpm import _sigmoid_beta_schedule
    ac = torch.cumprod(1.0 - _sigmoid_beta_schedule(T), 0)
    return torch.sqrt(ac).float(), torch.sqrt(1.0 - ac).float()


# ----------------------------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------------------------
# low-resolution maps that are no powers of two and leave the 8 x 16 tile partial; every output row and column of the 3 x 3 map
# touches a clamped edge; 9 x 17 (not asked for by name): four workgroups per sample, the second row / column of tiles one
# pixel wide, so every halo direction is read
SHAPES = [(5, 7, 2), (5, 7, 4), (3, 3, 8), (9, 17, 2), (9, 17, 4)]


@pytest.mark.parametrize("h,w,r", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_lowres_cond_kernel_against_the_float64_restatement(dev, parity, C, h, w, r):
    """Per element |kernel - float64| <= (k + 2) u M, k = lowres_ref.roundings(...) the roundings on the longest path in the
    kernel's order - 2 log2 r for the two halving trees of the average (training source only), 1 for 2 l - 1, 4 for the
    bilinear taps (tap product, row sum, row product, column sum; exact weights), 2 for the augmentation (product, sum) - and
    M the sum of the magnitudes of the terms: derived, not measured.  B = 3 with s = (0, 517, 999), one level per sample."""
    from lgm_hip import ops
    B, H, W = 3, h * r, w * r
    pitch, off = (C + 3) // 4 * 4 * 2, 0 if C == 3 else 2          # C = 1: the slice in the middle of a pitch of 8
    g = torch.Generator().manual_seed(1000 * h + 10 * r + C)
    img = torch.rand(B, C, H, W, generator=g) * 3 - 1              # outside [0, 1] too: both signs after normalisation
    eps = torch.randn(B, C, H, W, generator=g)
    s = torch.tensor([0, 517, 999])
    sa, sb = _tables()
    sad, sbd, sd, imgd, epsd = sa.to(dev), sb.to(dev), s.to(dev), img.to(dev), eps.to(dev)
    low32 = LR.area_mean_f32(img, r)
    lowd = low32.to(dev)

    def run(**kw):
        buf = torch.full((B, H, W, pitch), SENTINEL, device=dev)
        ops.lowres_cond(buf, off, C, r, **kw)
        assert ops.lib()._dll.lgm_last_kernel().decode() == "lowres_cond_kernel"
        out = buf.cpu()
        keep = torch.ones(pitch, dtype=torch.bool)
        keep[off:off + C] = False
        assert bool((out[..., keep] == SENTINEL).all()), "a lane outside the slice was written"
        return out[..., off:off + C].permute(0, 3, 1, 2).contiguous()

    aug = dict(eps=epsd, s=sd, sqrt_ac=sad, sqrt_1mac=sbd)
    got = {}
    for src, kw, ref_kw in (("img", dict(img=imgd), dict(img=img)), ("low", dict(low=lowd), dict(low=low32))):
        for normalize in (True, False):
            for augment in (True, False):
                out = run(**kw, normalize=normalize, **(aug if augment else {}))
                got[src, normalize, augment] = out
                want, M = LR.cond_slice(r, normalize=normalize, **ref_kw,
                                        **(dict(sqrt_ac=sa, sqrt_1mac=sb, s=s, eps=eps) if augment else {}))
                k = LR.roundings(r, src == "img", normalize, augment)
                excess = ((out.double() - want).abs() - (k + 2) * U * M).max()
                worst = ((out.double() - want).abs() / M.clamp_min(1e-30)).max() / U
                parity.record(f"lowres_cond C={C} {h}x{w} r={r} {src} norm={int(normalize)} aug={int(augment)}: worst error in "
                              f"units of u M (bound {k + 2})", err_over_uM=worst, bound=k + 2)
                assert float(excess) <= 0, (src, normalize, augment, float(worst), k + 2)
    for normalize in (True, False):
        for augment in (True, False):
            assert torch.equal(got["img", normalize, augment], got["low", normalize, augment]), \
                "the two sources agree to the bit when low is the float32 average the training source forms"
    # eps = NULL: the unaugmented value, bit for bit - also where s and the tables are handed in and s = 0 is no special row
    u = got["img", True, False]
    assert not torch.equal(got["img", True, True][0], u[0]), "s = 0 still augments: sqrt_1mac[0] is not zero"
    # s outside the table is clamped on the device
    wild = run(img=imgd, normalize=True, eps=epsd, s=torch.tensor([-5, 517, 2 ** 40], device=dev), sqrt_ac=sad, sqrt_1mac=sbd)
    assert torch.equal(wild, got["img", True, True])
    # a second launch gives the same bits (no atomics, fixed order)
    assert torch.equal(run(img=imgd, normalize=True, **aug), got["img", True, True])


def test_lowres_cond_at_the_flagship_shape_and_many_channels(dev):
    """128 x 128 from 32 x 32 (B = 2: 2 x 2 full tiles per sample) and a C = 64 slice (the LDS limit) at 16 x 32, r = 2"""
    from lgm_hip import ops
    sa, sb = _tables()
    for B, C, h, w, r in ((2, 3, 32, 32, 4), (1, 64, 8, 16, 2)):
        g = torch.Generator().manual_seed(C)
        img, eps = torch.rand(B, C, h * r, w * r, generator=g), torch.randn(B, C, h * r, w * r, generator=g)
        s = torch.randint(0, 1000, (B,), generator=g)
        pitch = 2 * ((C + 3) // 4 * 4)
        buf = torch.full((B, h * r, w * r, pitch), SENTINEL, device=dev)
        ops.lowres_cond(buf, 0, C, r, img=img.to(dev), eps=eps.to(dev), s=s.to(dev), sqrt_ac=sa.to(dev), sqrt_1mac=sb.to(dev),
                        normalize=True)
        out = buf.cpu()
        assert bool((out[..., C:] == SENTINEL).all())
        want, M = LR.cond_slice(r, img=img, normalize=True, sqrt_ac=sa, sqrt_1mac=sb, s=s, eps=eps)
        k = LR.roundings(r, True, True, True)
        assert float(((out[..., :C].permute(0, 3, 1, 2).double() - want).abs() - (k + 2) * U * M).max()) <= 0


@pytest.mark.parametrize("B,td", [(1, 64), (3, 256), (130, 64)])
def test_lowres_emb_add_kernel(dev, B, td):
    """temb' = fl(temb + e): one rounding; st = SiLU(temb') as lgm_label_emb_fwd computes it, the bound of its test"""
    from lgm_hip import ops
    g = torch.Generator().manual_seed(B + td)
    temb0, add = torch.randn(B, td, generator=g) * 3, torch.randn(B, td, generator=g)
    temb, st = temb0.to(dev), torch.full((B, td), SENTINEL, device=dev)
    ops.lowres_emb_fwd(temb, st, add.to(dev))
    assert ops.lib()._dll.lgm_last_kernel().decode() == "lowres_emb_add_kernel"
    z = temb0.double() + add.double()
    sl = z / (1 + (-z).exp())
    assert float(((temb.cpu().double() - z).abs() - U * z.abs()).max()) <= 0
    assert float(((st.cpu().double() - sl).abs() - 8 * U * (z.abs() + sl.abs())).max()) <= 0
    again, keep = temb0.to(dev), torch.full((B, td), SENTINEL, device=dev)
    ops.lowres_emb_fwd(again, None, add.to(dev))
    assert torch.equal(again, temb) and bool((keep == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# the constant slice survives a chain
# ----------------------------------------------------------------------------------------------------------------------
def _small(dev, C=3, **kw):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    torch.manual_seed(3)
    net = Unet(dim=16, channels=C, lowres_cond=True, **{k: kw.pop(k) for k in ("num_classes", "dropout") if k in kw})
    gd = GaussianDiffusion(net, img_size=16, **kw).to(dev)
    net.prepare_hip(dev)
    return gd


SAMPLERS = {"ddim": dict(timesteps=1000, sampling_timesteps=6, ddim_sampling_eta=0.5), "ancestral": dict(timesteps=6),
            "dpm++": dict(timesteps=1000, sampling_timesteps=6, sampler="dpm++", dpm_stochastic=True)}


def _plan(gd):
    from lgm_hip import sampler
    return {"dpm": sampler._plan_dpm, "ddim": sampler._plan_ddim, "ancestral": sampler._plan_ancestral}[sampler._sampler_kind(gd)](gd)


@pytest.mark.parametrize("dyn", [False, True], ids=["clamp", "dynthresh"])
@pytest.mark.parametrize("kind", list(SAMPLERS))
@pytest.mark.parametrize("C", [3, 1])
def test_conditioning_slice_survives_a_chain(dev, monkeypatch, C, kind, dyn):
    """6 steps, eager launches and graph replay: the slice holds the bits ``lgm_lowres_cond`` gave it, x moved, pads are zero,
    and both ways give the same image."""
    from lgm_hip import ops, sampler
    gd = _small(dev, C, dynamic_thresholding=dyn, **SAMPLERS[kind])
    net, B = gd.model, 2
    shape = (B, C, 16, 16)
    g = torch.Generator().manual_seed(5)
    low, eps = torch.rand(B, C, 4, 4, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    init = torch.randn(shape, generator=g).to(dev)
    s = torch.tensor([3, 2], device=dev) if kind == "ancestral" else torch.tensor([0, 700], device=dev)
    want = torch.full((B, 16, 16, net.in_pitch), SENTINEL, device=dev)
    ops.lowres_cond(want, net.cond_off, C, 4, low=low, eps=eps, s=s, sqrt_ac=gd.sqrt_alphas_cumprod,
                    sqrt_1mac=gd.sqrt_one_minus_alphas_cumprod, normalize=True)
    want = net.cond_slice(want).clone()
    plan = _plan(gd)
    assert len(plan.times) == 6
    noises = [torch.randn(shape, generator=g).to(dev) if d else None for d in plan.draws]
    lr = dict(lowres=low, lowres_aug_t=s, lowres_noise=eps)
    # eager
    chain = sampler._Chain(gd, shape, init, **lr)
    x_first = net.x_slice(chain.x).clone()
    assert torch.equal(net.cond_slice(chain.x), want)
    for t, row, nz in zip(plan.times, plan.rows, noises):
        chain.step(t, nz, row, plan.rederive, plan.dpm)
    assert torch.equal(net.cond_slice(chain.x), want), "eager chain: the conditioning slice changed"
    assert not torch.equal(net.x_slice(chain.x), x_first) and torch.isfinite(chain.x).all()
    assert int(torch.count_nonzero(chain.x[..., net.x_off + C:])) == 0, "pad lanes behind x are zero"
    eager = chain.image(True)
    # graph replay
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    img = sampler._run(gd, shape, plan, init_noise=init, noises=noises, lowres=lr)
    ents = [e for k, e in sampler._GRAPHS[net].items() if isinstance(e, sampler._GraphedChain)]
    assert len(ents) == 1 and "lowres" in next(iter(sampler._GRAPHS[net])), "graph capture of the conditioned step did not happen"
    assert torch.equal(net.cond_slice(ents[0].x), want), "replayed chain: the conditioning slice changed"
    assert torch.equal(ents[0].lowres_s, s)
    assert torch.equal(img, eager), "graph replay differs from eager launches"


def test_sample_api_and_cascade(dev):
    from models.generative.diffusion.ddpm import DDPM, sample_cascade
    gd = _small(dev, timesteps=6, lowres_sample_aug_t=2)
    low = torch.rand(2, 3, 4, 4, device=dev)
    torch.manual_seed(4)
    a = gd.sample(lowres=low)                                   # batch from the image, level 2 from the constructor
    torch.manual_seed(4)
    b = gd.sample(batch_size=2, lowres=low, lowres_aug_t=2)
    torch.manual_seed(4)
    c = gd.sample(lowres=low, lowres_aug_t=torch.tensor([2, 5]))
    torch.manual_seed(4)
    d = gd.sample(lowres=low.flip(0))
    assert a.shape == (2, 3, 16, 16) and torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]) and not torch.equal(a, d)
    out = gd.sample(lowres=low, return_all_timesteps=True)
    assert out.shape == (2, 7, 3, 16, 16) and torch.isfinite(out).all()
    x = torch.rand(2, 3, 16, 16, device=dev) * 2 - 1
    img, x0 = gd.p_sample(x, 3, lowres=low)
    assert torch.isfinite(img).all() and float(x0.abs().max()) <= 1.0
    torch.manual_seed(6)
    base = DDPM(img_size=8, dim=16, diffusion_timesteps=4)
    sr = DDPM(img_size=16, dim=16, diffusion_timesteps=4, lowres_cond=True, lowres_factor=2)
    for m in (base, sr):
        m.to(dev)
        m.prepare_hip(dev)
    big = sample_cascade([base, sr], 3)
    assert big.shape == (3, 3, 16, 16) and torch.isfinite(big).all()
    assert torch.isfinite(sr.upsample(torch.rand(1, 3, 8, 8, device=dev))).all()


# ----------------------------------------------------------------------------------------------------------------------
# parity with the reference's self-conditioned modules fed the conditioning image (dim 16, 16 x 16, r = 4, B = 4)
# ----------------------------------------------------------------------------------------------------------------------
def _params(fx, label=False):
    from oracle import diffusion as OD
    P = OD.unet_init(dim=int(fx["dim"]), channels=3, seed=int(fx["seed"]))
    P["init_conv.weight"] = torch.as_tensor(fx["init_conv.weight"])
    for n in ("1.weight", "1.bias", "3.weight", "3.bias"):
        P[f"lowres_time_mlp.{n}"] = torch.as_tensor(fx[f"lowres_time_mlp.{n}"])
    if label:
        P["label_emb.weight"] = torch.as_tensor(fx["label_emb.weight"])
    return P


class _Case:
    def __init__(self, fx, objective, dev):
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        self.o, self.dev = objective, dev
        self.S, self.B, self.r = int(fx["S"]), int(fx["B"]), int(fx["r"])
        g = torch.Generator().manual_seed(int(fx["data_seed"]))
        self.img = torch.rand(self.B, 3, self.S, self.S, generator=g)
        self.noise = torch.randn(self.B, 3, self.S, self.S, generator=g)
        self.eps = torch.randn(self.B, 3, self.S, self.S, generator=torch.Generator().manual_seed(int(fx["aug_seed"])))
        self.t, self.s = torch.as_tensor(fx["t"]), torch.as_tensor(fx["s"])
        self.net = Unet(dim=int(fx["dim"]), channels=3, lowres_cond=True)
        self.net.load_state_dict(_params(fx), strict=True)
        self.mk = lambda **kw: GaussianDiffusion(self.net, img_size=self.S, objective=objective, lowres_factor=self.r,
                                                 **kw).to(dev)
        self.gd = self.mk(timesteps=1000, sampling_timesteps=int(fx["ddim_steps"]))
        self.net.prepare_hip(dev)
        self.fx = {k[len(objective) + 1:]: v for k, v in fx.items() if k.startswith(objective + ":")}


@pytest.fixture(scope="module", params=["pred_v", "pred_noise"])
def case(request, fx, dev):
    return _Case(fx, request.param, dev)


def _arbiter(parity, what, hip, ref, exact=None):
    """1e-4 against the reference's fp32 result; with ``exact`` (the fixture's float64 evaluation) a miss is decided by float64 -
    HIP no further from it than twice the reference itself.  Both distances to float64 go on record either way."""
    e = rel(hip, ref)
    if exact is not None:
        parity.record(what + " [distances to float64]", hip_vs_ref=e, ref_vs_fp64=rel(ref, exact), hip_vs_fp64=rel(hip, exact))
    if e < RTOL or exact is None:
        return parity(what, e, RTOL)
    d_ref, d_hip = rel(ref, exact), rel(hip, exact)
    print(f"[parity] {what}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, hip {d_hip:.3e}")
    assert d_hip <= 2 * d_ref, (what, e, d_hip, d_ref)


def test_unet_output_matches_reference_fixture(case, parity):
    net, dev = case.net, case.dev
    x, t, s = torch.as_tensor(case.fx["x_t"]).to(dev), case.t.to(dev), case.s.to(dev)
    cond = torch.as_tensor(case.fx["cond"]).to(dev)
    with torch.no_grad():
        out = net(x, t, lowres_cond_img=cond, lowres_aug_t=s)
        zero = net(x, t, lowres_cond_img=cond)
        other = net(x, t, lowres_cond_img=cond.flip(0), lowres_aug_t=s)
    parity(f"{case.o}: unet_out, s {tuple(case.s.tolist())}", rel(out, case.fx["unet_out"]), RTOL)
    assert torch.equal(out[0], zero[0]), "lowres_aug_t=None is level 0: sample 0 carries it in both"
    assert rel(out[1:], zero[1:]) > 1e-3 and rel(out, other) > 1e-2, "the level and the image reach the output"


def test_training_step_matches_reference_fixture(case, parity):
    gd, net, dev, fx = case.gd, case.net, case.dev, case.fx
    net._flat.zero_grad()
    loss = gd.p_losses(case.img.to(dev), case.t.to(dev), case.noise.to(dev), _normalize=True, lowres_aug_t=case.s.to(dev),
                       lowres_noise=case.eps.to(dev))
    want = float(fx["loss"])
    parity(f"{case.o}: loss", abs(loss.item() - want) / want, RTOL)
    loss.backward()
    sd = dict(net.named_parameters())
    gw = sd["init_conv.weight"].grad
    parity(f"{case.o}: init_conv.weight gradient, conditioning half", rel(gw[:, :3], fx["grad:init_conv.weight"][:, :3]), RTOL)
    parity(f"{case.o}: init_conv.weight gradient, x half", rel(gw[:, 3:], fx["grad:init_conv.weight"][:, 3:]), RTOL)
    for n in ("1.weight", "1.bias", "3.weight", "3.bias"):
        parity(f"{case.o}: lowres_time_mlp.{n} gradient", rel(sd[f"lowres_time_mlp.{n}"].grad, fx[f"grad:lowres_time_mlp.{n}"]), RTOL)
    worst, worst_n, worst_s, seen = 0.0, 0.0, 0.0, set()
    Ks = 1024
    for k in fx:
        if k.startswith("grad:"):
            worst = max(worst, rel(sd[k[5:]].grad, fx[k]))
            seen.add(k[5:])
        elif k.startswith("gradnorm:"):
            n = k[9:]
            worst_n = max(worst_n, abs(sd[n].grad.double().norm().item() - float(fx[k])) / max(float(fx[k]), 1e-12))
            flat = sd[n].grad.reshape(-1)
            worst_s = max(worst_s, rel(flat[:: flat.numel() // Ks][:Ks], fx["gradsample:" + n]))
            seen.add(n)
    assert len(seen) == 30, "the 26 tensors of the other fixtures and lowres_time_mlp's four"
    parity(f"{case.o}: worst parameter gradient (whole tensors)", worst, RTOL)
    parity(f"{case.o}: worst gradient norm (large tensors)", worst_n, RTOL)
    parity(f"{case.o}: worst 1024-element gradient sample (large tensors)", worst_s, RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    parity(f"{case.o}: all-parameter gradient norm", abs(gn - float(fx["gradnorm_all"])) / float(fx["gradnorm_all"]), RTOL)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    net._flat.zero_grad()


def _chains(case, fx):
    from lgm_hip import sampler
    from oracle import diffusion as OD
    dev, shape = case.dev, (case.B, 3, case.S, case.S)
    low = torch.as_tensor(fx["low"]).to(dev)
    out = {}
    init, nz = OD.draw_loop_noise(int(fx["ddim_loop_seed"]), shape, int(fx["ddim_steps"]) - 1)
    out["ddim_loop"] = sampler.ddim_sample(case.gd, shape, init_noise=init.to(dev), noises=[x.to(dev) for x in nz] + [None],
                                           lowres=dict(lowres=low, lowres_aug_t=case.s.to(dev),
                                                       lowres_noise=case.eps.to(dev))).clone()
    T = int(fx["ancestral_T"])
    gda = case.mk(timesteps=T)
    init, nz = OD.draw_loop_noise(int(fx["p_sample_loop_seed"]), shape, T - 1)
    out["p_sample_loop"] = sampler.p_sample_loop(gda, shape, init_noise=init.to(dev), noises=[x.to(dev) for x in nz] + [None],
                                                 lowres=dict(lowres=low, lowres_aug_t=torch.as_tensor(fx["s_ancestral"]).to(dev),
                                                             lowres_noise=case.eps.to(dev))).clone()
    return out


def test_chains_match_reference_fixture_and_graph_replay_equals_eager(case, fx, parity, monkeypatch):
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = _chains(case, fx)
    again = _chains(case, fx)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = _chains(case, fx)
    for k, what in (("ddim_loop", "20-pair DDIM chain"), ("p_sample_loop", "50-step ancestral chain")):
        assert torch.isfinite(graph[k]).all() and float(graph[k].std()) > 0
        assert torch.equal(graph[k], eager[k]), f"{what}: graph replay differs from eager launches"
        assert torch.equal(graph[k], again[k]), f"{what}: the second chain on one captured step differs from the first"
        _arbiter(parity, f"{case.o}: {what}, final image", graph[k], case.fx[k], case.fx[k + "64"])


def test_guided_class_conditional_stage_matches_reference_fixture(fx, dev, parity):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    net = Unet(dim=16, channels=3, lowres_cond=True, num_classes=int(fx["K"]))
    net.load_state_dict(_params(fx, label=True), strict=True)
    gd = GaussianDiffusion(net, img_size=16, timesteps=1000, objective="pred_v").to(dev)
    net.prepare_hip(dev)
    x, cond = torch.as_tensor(fx["pred_v:x_t"]).to(dev), torch.as_tensor(fx["pred_v:cond"]).to(dev)
    t, s, y = (torch.as_tensor(fx[k]).to(dev) for k in ("t", "s", "classes"))
    with torch.no_grad():
        out = net(x, t, classes=y, lowres_cond_img=cond, lowres_aug_t=s)
        mp = gd.model_predictions(x, t, classes=y, cond_scale=float(fx["cond_scale"]), lowres_cond_img=cond, lowres_aug_t=s)
    parity("guided stage: conditional unet_out", rel(out, fx["guided:unet_out:cond"]), RTOL)
    _arbiter(parity, "guided stage: unclipped x_start at cond_scale 3", mp.pred_x_start, fx["guided:x_start"], fx["guided:x_start64"])
    # a guided chain runs, replayed and eager alike
    low = torch.rand(4, 3, 4, 4, device=dev)
    g6 = GaussianDiffusion(net, img_size=16, timesteps=6, objective="pred_v", cond_scale=3.0).to(dev)
    torch.manual_seed(2)
    a = g6.sample(lowres=low, classes=y)
    os.environ["LGM_NO_SAMPLER_GRAPH"] = "1"
    try:
        torch.manual_seed(2)
        b = g6.sample(lowres=low, classes=y)
    finally:
        os.environ.pop("LGM_NO_SAMPLER_GRAPH")
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# the graph-replayed training step, the random stream of a plain model, train.py
# ----------------------------------------------------------------------------------------------------------------------
def _module(dev, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(img_size=16, dim=16, lr=1e-3, ema_update_every=2, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("kw,acc", [(dict(), 1), (dict(dropout=0.1, objective="pred_noise"), 2)], ids=["plain_step", "accumulate2_dropout"])
def test_graph_replayed_training_step_equals_eager_steps(dev, kw, acc):
    """Four steps through ``make_fast_step``, s and eps_aug drawn inside the graph from the same seeded device generator: losses,
    parameters after Adam, the EMA shadow and the Adam state of graph replay and eager launches are the same bits; two replays
    draw different s and eps_aug."""
    a, b = _module(dev, lowres_cond=True, **kw), _module(dev, lowres_cond=True, **kw)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True, accumulate=acc), b.make_fast_step(ob, 1, False, accumulate=acc)
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(8, 3, 16, 16, generator=g).to(dev) for _ in range(4)]
    y = torch.zeros(8, dtype=torch.long, device=dev)
    losses, drawn = {}, []
    for name, fast in (("graph", fa), ("eager", fb)):
        torch.manual_seed(77)
        losses[name] = []
        for i, x in enumerate(xs):
            losses[name].append(fast.step((x.clone(), y), i).detach().clone().reshape(()))
            if name == "graph":
                drawn.append((fast.graphed.lowres_s.clone(), fast.graphed.lowres_noise.clone()))
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    for la, lb in zip(losses["graph"], losses["eager"]):
        assert torch.isfinite(la) and torch.equal(la, lb), (float(la), float(lb))
    assert not torch.equal(drawn[0][0], drawn[1][0]) and not torch.equal(drawn[0][1], drawn[1][1]), "every replay draws anew"
    assert all(int(s.min()) >= 0 and int(s.max()) < 1000 for s, _ in drawn)
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data)
    assert torch.equal(a.ema.ema_model.model._flat.data, b.ema.ema_model.model._flat.data)
    w0 = _module(dev, lowres_cond=True, **kw).ema.online_model.model.lowres_time_mlp[3].weight
    assert not torch.equal(na.lowres_time_mlp[3].weight, w0), "lowres_time_mlp trains"
    for pa, pb in zip(oa.state_dict()["state"].values(), ob.state_dict()["state"].values()):
        for k in pb:
            assert torch.equal(torch.as_tensor(pa[k]), torch.as_tensor(pb[k])), k


def test_a_plain_models_random_stream_is_untouched(dev):
    """For one seed a plain and a conditioned model draw the same first t and noise (the new draws stand behind them), in the
    captured step and in eager ``forward``; the plain model draws nothing more: its generator ends where it ended."""
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    x = torch.rand(8, 3, 16, 16, device=dev)
    y = torch.zeros(8, dtype=torch.long, device=dev)
    got = {}
    for name, kw in (("plain", {}), ("cond", dict(lowres_cond=True))):
        m = _module(dev, **kw)
        fast = m.make_fast_step(m.configure_optimizers(), 1, True)
        torch.manual_seed(123)
        fast.step((x.clone(), y), 0)
        assert fast.mode.startswith("hipGraph")
        got[name] = (fast.graphed.t.clone(), fast.graphed.noise.clone(), fast.graphed.lowres_s)
    assert torch.equal(got["plain"][0], got["cond"][0]) and torch.equal(got["plain"][1], got["cond"][1])
    assert got["plain"][2] is None and got["cond"][2] is not None
    # eager forward: t ~ randint, noise ~ randn and nothing else on a plain model
    torch.manual_seed(3)
    net = Unet(dim=16)
    gd = GaussianDiffusion(net, img_size=16).to(dev)
    net.prepare_hip(dev)
    torch.manual_seed(55)
    with torch.no_grad():
        gd(x)
    after = torch.rand(4, device=dev)
    torch.manual_seed(55)
    torch.randint(0, 1000, (8,), device=dev)
    torch.randn_like(x)
    assert torch.equal(after, torch.rand(4, device=dev))


def test_train_entry_runs_the_sr_config(tmp_path):
    """train.py's main() on configs/diffusion/ddpm_sr_32_128.json at a reduced size (16 x 16 from 4 x 4, dim 16, 20 diffusion
    steps: the step-0 sample super-resolves the first batch, downsampled), six steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "ddpm_sr_32_128.json")))
    assert cfg["model"]["args"]["lowres_cond"] is True and cfg["model"]["args"]["lowres_factor"] == 4
    cfg["model"]["args"].update(img_size=16, dim=16, diffusion_timesteps=20)
    cfg["dataset"].update(img_size=16, batch_size=8)
    path = tmp_path / "ddpm_sr_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_ddpm_sr"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('LAST_SAMPLES', tuple(m.last_samples.shape), bool(torch.isfinite(m.last_samples).all())); "
            "print('TRAIN_LOSS', float(m.logged['train_loss']))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "6", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("LAST_SAMPLES", "TRAIN_LOSS"))}
    assert lines["LAST_SAMPLES"] == "LAST_SAMPLES (8, 3, 16, 16) True", lines
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 6 and sd["hyper_parameters"]["lowres_cond"] is True
    assert tuple(sd["state_dict"]["ema.online_model.model.lowres_time_mlp.3.weight"].shape) == (64, 64)
    assert tuple(sd["state_dict"]["ema.online_model.model.init_conv.weight"].shape) == (16, 6, 7, 7)
    for v in sd["state_dict"].values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
