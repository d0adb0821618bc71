"""GPU: the class-conditional DDPM with classifier-free guidance (``Unet(num_classes=K)``; an extension of the reference).

  * the three kernels of csrc/classcond.hip alone: the forward against float64 (bound below), the weight gradient bit for bit
    against a float32 loop in ascending sample order, the guidance mix on pitch-4 buffers with sentinel pad lanes;
  * UNet outputs, training step, model_predictions and a self-conditioned case against what the REFERENCE's modules returned
    with a label embedding added to their time embedding (tests/golden/diffusion_classcond.npz, written by
    tools/make_golden_classcond.py), 1e-4 relative; an unclipped x_start or a guided chain that misses 1e-4 is decided by the
    float64 arbiter rule of tests/test_hip_objectives.py (HIP no further from the fixture's float64 evaluation than twice the
    reference is);
  * graph replay bit for bit against eager launches (guided chains, training step with in-graph label drop), cond_scale = 1
    against the single conditional forward, FusedAdam / EMA / checkpoints, train.py on configs/diffusion/ddpm_cond.json.

Measured distances go through the ``parity`` recorder (committed record: profiles/r09_classcond_parity.json).
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
    return dict(np.load(os.path.join(golden_dir, "diffusion_classcond.npz")))


# ----------------------------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------------------------
def _label_sets(g, B, K):
    """random labels in [0, K], all the same class, all null, and (B < K + 1 or forced) a class no sample has"""
    rnd = torch.randint(0, K + 1, (B,), generator=g)
    rnd[rnd == 0] = K                                          # class 0 is the one no sample has
    return {"random, none of class 0": rnd, "all the same": torch.full((B,), K - 1, dtype=torch.long),
            "all null": torch.full((B,), K, dtype=torch.long)}


@pytest.mark.parametrize("td", [64, 256])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_label_emb_forward_kernel(dev, B, td):
    """temb' = fl(temb + e) is one rounding: |error| <= u |temb + e|.  st = z / (1 + exp(-z)) at z = temb': the input's
    rounding moves it by at most |silu'| u |z| <= 1.1 u |z|, exp, the sum and the quotient add about 4 u |st|; asserted
    against 8 u (|z| + |st|), the margin of tests/test_hip_selfcond.py."""
    from lgm_hip import ops
    for K in (1, 5, 1000):
        g = torch.Generator().manual_seed(B * 1000 + td + K)
        emb = torch.randn(K + 1, td, generator=g)
        temb0 = torch.randn(B, td, generator=g) * 3
        embd = emb.to(dev)
        for what, y in _label_sets(g, B, K).items():
            temb, st = temb0.to(dev), torch.full((B, td), SENTINEL, device=dev)
            ops.label_emb_fwd(temb, st, embd.data_ptr(), y.to(dev), K)
            assert ops.lib()._dll.lgm_last_kernel().decode() == "label_emb_fwd_kernel"
            z = temb0.double() + emb[y].double()
            s = z / (1 + (-z).exp())
            assert float(((temb.cpu().double() - z).abs() - U * z.abs()).max()) <= 0, (K, what)
            assert float(((st.cpu().double() - s).abs() - 8 * U * (z.abs() + s.abs())).max()) <= 0, (K, what)
    # labels the host could not see are clamped into [0, K]
    temb, st = temb0.to(dev), torch.empty(B, td, device=dev)
    wild = torch.full((B,), 2 ** 40, dtype=torch.long)
    wild[0] = -3
    ops.label_emb_fwd(temb, st, embd.data_ptr(), wild.to(dev), K)
    want = temb0.clone()
    want[0] += emb[0]
    want[1:] += emb[K]
    assert torch.equal(temb.cpu(), want)


@pytest.mark.parametrize("td", [64, 256])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_label_emb_weight_gradient_kernel_is_the_ascending_float32_sum(dev, B, td):
    from lgm_hip import ops
    for K in (1, 5, 1000):
        g = torch.Generator().manual_seed(B * 1000 + td + K + 1)
        gt = torch.randn(B, td, generator=g)
        old = torch.randn(K + 1, td, generator=g)
        for what, y in _label_sets(g, B, K).items():
            for beta in (0.0, 1.0):
                acc = torch.zeros(K + 1, td)
                for b in range(B):                             # float32, ascending b
                    acc[int(y[b])] = acc[int(y[b])] + gt[b]
                want = acc if beta == 0.0 else old * beta + acc
                absent = torch.ones(K + 1, dtype=torch.bool)
                absent[y] = False
                assert absent.any()
                out = old.to(dev)
                ops.label_emb_wgrad(gt.to(dev), y.to(dev), out.data_ptr(), beta, K)
                assert ops.lib()._dll.lgm_last_kernel().decode() == "label_emb_wgrad_kernel"
                out = out.cpu()
                assert torch.equal(out, want), (K, what, beta)
                assert torch.equal(out[absent], old[absent] * beta), "rows no sample has: exactly beta x the old value"


@pytest.mark.parametrize("C", [3, 1])
def test_cfg_mix_kernel(dev, C):
    """105 pixels (B = 3, 5 x 7: a partial last block), pitch 4.  Three roundings (difference, product, sum), each at most u
    relative to its partial result: |error| <= 3 u M with M = |null| + s |cond - null|; asserted against 8 u M."""
    from lgm_hip import ops
    g = torch.Generator().manual_seed(90 + C)
    rows = 3 * 5 * 7
    cond = torch.full((3, 5, 7, 4), SENTINEL)
    null = torch.full((3, 5, 7, 4), -SENTINEL)
    cond[..., :C] = torch.randn(3, 5, 7, C, generator=g)
    null[..., :C] = torch.randn(3, 5, 7, C, generator=g)
    nd = null.to(dev)
    for s in (0.0, 1.0, 3.0):
        out = cond.to(dev)
        ops.cfg_mix(out, nd, s, C)
        assert ops.lib()._dll.lgm_last_kernel().decode() == "cfg_mix_kernel"
        out2 = cond.to(dev)
        ops.cfg_mix(out2, nd, 123.0, C, scale_dev=torch.tensor([s], device=dev))   # the scale a captured step reads
        assert torch.equal(out, out2), "scale from the device buffer: the same bits"
        assert torch.equal(nd.cpu(), null), "the null output is read only"
        out = out.cpu()
        assert torch.equal(out[..., C:], cond[..., C:]), "pad lanes keep their value"
        if s == 1.0:
            assert torch.equal(out, cond)
        elif s == 0.0:
            assert torch.equal(out[..., :C], null[..., :C])
        else:
            c, n = cond[..., :C].double(), null[..., :C].double()
            m = n.abs() + s * (c - n).abs()
            assert float(((out[..., :C].double() - (n + s * (c - n))).abs() - 8 * U * m).max()) <= 0
    assert rows % 256 != 0


# ----------------------------------------------------------------------------------------------------------------------
# parity with the reference's modules + label embedding (dim 16, 16 x 16, K = 5, classes (3, 0, 3, 5), t = (37, 912, 0, 999))
# ----------------------------------------------------------------------------------------------------------------------
def _params(fx):
    from oracle import diffusion as OD
    P = OD.unet_init(dim=int(fx["dim"]), channels=3, seed=int(fx["seed"]))
    P["label_emb.weight"] = torch.as_tensor(fx["label_emb.weight"])
    return P


class _Case:
    def __init__(self, fx, objective, dev):
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        self.o, self.dev = objective, dev
        self.dim, self.S, self.B, self.K = int(fx["dim"]), int(fx["S"]), int(fx["B"]), int(fx["K"])
        g = torch.Generator().manual_seed(int(fx["data_seed"]))
        self.img = torch.rand(self.B, 3, self.S, self.S, generator=g)
        self.noise = torch.randn(self.B, 3, self.S, self.S, generator=g)
        self.t = torch.as_tensor(fx["t"])
        self.classes = torch.as_tensor(fx["classes"])
        self.scale = float(fx["cond_scale"])
        self.net = Unet(dim=self.dim, channels=3, num_classes=self.K)
        self.net.load_state_dict(_params(fx), strict=True)
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
    unclipped x_start only) a miss is decided by float64 - HIP no further from it than twice the reference itself.  Both
    distances to float64 go on record either way."""
    e = rel(hip, ref)
    if exact is not None:
        parity.record(what + " [distances to float64]", hip_vs_ref=e, ref_vs_fp64=rel(ref, exact), hip_vs_fp64=rel(hip, exact))
    if e < RTOL or exact is None:
        return parity(what, e, RTOL)
    d_ref, d_hip = rel(ref, exact), rel(hip, exact)
    print(f"[parity] {what}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, hip {d_hip:.3e}")
    assert d_hip <= 2 * d_ref, (what, e, d_hip, d_ref)


def test_unet_outputs_match_reference_fixture(case, parity):
    net, dev = case.net, case.dev
    x, t, y = case.x_t.to(dev), case.t.to(dev), case.classes.to(dev)
    with torch.no_grad():
        cond, none = net(x, t, classes=y), net(x, t)
        null = net(x, t, classes=torch.full_like(y, case.K))
        host = net(x, t, classes=case.classes)                 # labels the host can see are checked, then copied
    parity(f"{case.o}: unet_out, classes {tuple(case.classes.tolist())}", rel(cond, case.fx["unet_out:cond"]), RTOL)
    parity(f"{case.o}: unet_out, all-null labels", rel(none, case.fx["unet_out:null"]), RTOL)
    assert torch.equal(none, null), "classes=None is the null label for every sample"
    assert torch.equal(host, cond)
    assert rel(cond, none) > 1e-2, "the labels reach the output"
    assert torch.equal(cond[3], none[3]), "sample 3 carries the null label in both"


def test_training_step_matches_reference_fixture(case, parity):
    gd, net, dev, fx = case.gd, case.net, case.dev, case.fx
    x0, noise = (case.img * 2 - 1).to(dev), case.noise.to(dev)
    net._flat.zero_grad()
    loss = gd.p_losses(x0, case.t.to(dev), noise, classes=case.classes.to(dev))
    want = float(fx["loss"])
    parity(f"{case.o}: loss", abs(loss.item() - want) / want, RTOL)
    loss.backward()
    sd = dict(net.named_parameters())
    ge = sd["label_emb.weight"].grad
    parity(f"{case.o}: label_emb.weight gradient [6, 64]", rel(ge, fx["grad:label_emb.weight"]), RTOL)
    assert int(torch.count_nonzero(ge[[1, 2, 4]])) == 0, "rows of the classes no sample has: exactly zero"
    assert all(float(ge[k].abs().max()) > 0 for k in (0, 3, 5))
    worst, worst_n, worst_s, n_seen = 0.0, 0.0, 0.0, 0
    Ks = 1024
    for k in fx:
        if k.startswith("grad:") and k != "grad:label_emb.weight":
            worst = max(worst, rel(sd[k[5:]].grad, fx[k]))
            n_seen += 1
        elif k.startswith("gradnorm:"):
            n = k[9:]
            worst_n = max(worst_n, abs(sd[n].grad.double().norm().item() - float(fx[k])) / max(float(fx[k]), 1e-12))
            flat = sd[n].grad.reshape(-1)
            worst_s = max(worst_s, rel(flat[:: flat.numel() // Ks][:Ks], fx["gradsample:" + n]))
            n_seen += 1
    assert n_seen == 26
    parity(f"{case.o}: worst parameter gradient (23 whole tensors)", worst, RTOL)
    parity(f"{case.o}: worst gradient norm (3 large tensors)", worst_n, RTOL)
    parity(f"{case.o}: worst 1024-element gradient sample (3 large tensors)", worst_s, RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    parity(f"{case.o}: all-parameter gradient norm", abs(gn - float(fx["gradnorm_all"])) / float(fx["gradnorm_all"]), RTOL)
    # accumulating pass (beta = 1): twice the gradient, absent rows still exactly zero
    g1 = ge.clone()
    gd.p_losses(x0, case.t.to(dev), noise, classes=case.classes.to(dev)).backward()
    ge = dict(net.named_parameters())["label_emb.weight"].grad
    assert torch.equal(ge, g1 + g1) and int(torch.count_nonzero(ge[[1, 2, 4]])) == 0
    net._flat.zero_grad()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("scale", [1, 3])
def test_model_predictions_match_reference_fixture(case, parity, scale, clip):
    dev = case.dev
    x, t, y = case.x_t.to(dev), case.t.to(dev), case.classes.to(dev)
    pred = case.gd.model_predictions(x, t, None, clip_x_start=clip, classes=y, cond_scale=float(scale))
    key = f"mp:s{scale}:{int(clip)}:"
    _arbiter(parity, f"{case.o}: pred_noise, cond_scale={scale}, clip={clip}", pred.pred_noise, case.fx[key + "pred_noise"])
    _arbiter(parity, f"{case.o}: pred_x_start, cond_scale={scale}, clip={clip}", pred.pred_x_start, case.fx[key + "x_start"],
             None if clip else case.fx[f"mp:s{scale}:0:x_start64"])
    if clip and scale == 3:                                    # p_mean_variance and p_sample take the keywords too
        mean, _, _, xs = case.gd.p_mean_variance(x, t, None, True, classes=y, cond_scale=3.0)
        assert torch.equal(xs, pred.pred_x_start) and torch.isfinite(mean).all()
        nz = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        img_a, xs_a = case.gd.p_sample(x, 500, None, noise=nz, classes=y, cond_scale=3.0)
        img_b, xs_b = case.gd.p_sample(x, 500, None, noise=nz, classes=y)
        assert float(xs_a.abs().max()) <= 1.0 and not torch.equal(img_a[:3], img_b[:3])
        assert torch.equal(img_a[3], img_b[3]), "a null-labelled sample is its own guidance target: scale s leaves it"


def test_self_conditioned_class_conditional_matches_reference_fixture(fx, dev, parity):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    P = _params(fx)
    P["init_conv.weight"] = torch.as_tensor(fx["sc:init_conv.weight"])
    net = Unet(dim=16, channels=3, self_condition=True, num_classes=int(fx["K"]))
    net.load_state_dict(P, strict=True)
    gd = GaussianDiffusion(net, img_size=16, timesteps=1000, objective="pred_v").to(dev)
    net.prepare_hip(dev)
    g = torch.Generator().manual_seed(int(fx["data_seed"]))
    img = torch.rand(4, 3, 16, 16, generator=g)
    noise = torch.randn(4, 3, 16, 16, generator=g)
    x0, n, t = (img * 2 - 1).to(dev), noise.to(dev), torch.as_tensor(fx["t"]).to(dev)
    y, sc = torch.as_tensor(fx["classes"]).to(dev), torch.as_tensor(fx["sc:x_self_cond"]).to(dev)
    with torch.no_grad():
        out = net(gd.q_sample(x0, t, n), t, sc, classes=y)
        loss = gd.p_losses(x0, t, n, classes=y, _self_cond=True)
        other = gd.p_losses(x0, t, n, _self_cond=True)
    parity("self-conditioned + classes: unet_out", rel(out, fx["sc:unet_out"]), RTOL)
    want = float(fx["sc:coin1:loss"])
    parity("self-conditioned + classes: loss, coin on", abs(loss.item() - want) / want, RTOL)
    assert abs(other.item() - want) / want > RTOL, "both passes read the labels"


# ----------------------------------------------------------------------------------------------------------------------
# guided sampling chains: reference fixture, graph replay against eager launches, cond_scale = 1
# ----------------------------------------------------------------------------------------------------------------------
def _gds(case, fx):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    n = int(fx["ddim_steps"])
    mk = lambda **kw: GaussianDiffusion(case.net, img_size=case.S, objective=case.o, **kw).to(case.dev)  # noqa: E731
    return {"ddim_loop": case.gd,
            "ddim_eta_loop": mk(timesteps=1000, sampling_timesteps=n, ddim_sampling_eta=float(fx["eta"])),
            "p_sample_loop": mk(timesteps=int(fx["ancestral_T"]))}


def _chains(case, fx, gds, scale, only=None):
    """the three chains of the fixture on the HIP engine -> {name: image}"""
    from lgm_hip import sampler
    from oracle import diffusion as OD
    dev, shape, out = case.dev, tuple(case.x_t.shape), {}
    y = case.classes.to(dev)
    for k in only or ("ddim_loop", "ddim_eta_loop", "p_sample_loop"):
        steps = int(fx["ancestral_T"]) if k == "p_sample_loop" else int(fx["ddim_steps"])
        init, nz = OD.draw_loop_noise(int(fx[k + "_seed"]), shape, steps - 1)
        fn = sampler.p_sample_loop if k == "p_sample_loop" else sampler.ddim_sample
        out[k] = fn(gds[k], shape, init_noise=init.to(dev), noises=[x.to(dev) for x in nz] + [None], classes=y,
                    cond_scale=scale).clone()
    return out


def test_guided_chains_match_reference_fixture_and_graph_replay_equals_eager(case, fx, parity, monkeypatch):
    from lgm_hip import sampler
    gds = _gds(case, fx)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = _chains(case, fx, gds, case.scale)
    per = sampler._GRAPHS[case.net]
    guided = [k for k, e in per.items() if "guided" in k and isinstance(e, sampler._GraphedChain)]
    assert len(guided) >= 2, "graph capture of the guided step did not happen"
    again = _chains(case, fx, gds, case.scale)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = _chains(case, fx, gds, case.scale)
    for k, what in (("ddim_loop", "20-pair guided DDIM chain, eta = 0"), ("ddim_eta_loop", "20-pair guided DDIM chain, eta = 0.7"),
                    ("p_sample_loop", "50-step guided ancestral chain")):
        assert torch.isfinite(graph[k]).all() and float(graph[k].std()) > 0
        assert torch.equal(graph[k], eager[k]), f"{what}: graph replay differs from eager launches"
        assert torch.equal(graph[k], again[k]), f"{what}: the second chain on one captured step differs from the first"
        _arbiter(parity, f"{case.o}: {what}, final image", graph[k], case.fx[k], case.fx[k + "64"])


def test_cond_scale_one_is_the_single_conditional_forward(case, fx, monkeypatch):
    """cond_scale = 1 runs the network once per step, cond_scale = 3 twice; two forwards mixed at scale 1 (the guided captured
    step with 1 in its scale buffer) give the single conditional forward's chain, bit for bit."""
    from lgm_hip import sampler
    gds = _gds(case, fx)
    calls = []
    real = case.net.forward_nhwc

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(case.net, "forward_nhwc", counting)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    n = int(fx["ddim_steps"])
    one = _chains(case, fx, gds, 1.0, only=("ddim_loop",))
    assert len(calls) == n, "one forward per step at cond_scale = 1"
    del calls[:]
    three = _chains(case, fx, gds, 3.0, only=("ddim_loop",))
    assert len(calls) == 2 * n
    assert not torch.equal(one["ddim_loop"], three["ddim_loop"])
    monkeypatch.setattr(case.net, "forward_nhwc", real)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    plain = _chains(case, fx, gds, 1.0, only=("ddim_loop", "p_sample_loop"))
    assert torch.equal(plain["ddim_loop"], one["ddim_loop"]), "graph replay of the single-forward step"
    # the guided captured step at scale 1: same labels, two forwards, lgm_cfg_mix keeps the conditional output
    from oracle import diffusion as OD
    dev, shape = case.dev, tuple(case.x_t.shape)
    for k, gd in (("ddim_loop", gds["ddim_loop"]), ("p_sample_loop", gds["p_sample_loop"])):
        anc = k == "p_sample_loop"
        steps = int(fx["ancestral_T"]) if anc else n
        init, nz = OD.draw_loop_noise(int(fx[k + "_seed"]), shape, steps - 1)
        chain = sampler._Chain(gd, shape, init.to(dev), None, case.classes.to(dev), 1.0)
        gc = sampler._graph_chain(gd, shape, anc, rederive=not anc, guided=True)
        assert gc is not None and gc.scale is not None
        noises = [x.to(dev) for x in nz] + [None]
        if anc:
            ts = list(reversed(range(gd.num_timesteps)))
            chain.x = gc.run(chain.x, ts, [sampler._p_sample_coeffs(gd, t) for t in ts], noises, chain.classes, 1.0)
        else:
            pairs = gd.ddim_time_pairs()
            chain.x = gc.run(chain.x, [a for a, _ in pairs], [sampler._ddim_coeffs(gd, a, b, 0.0) for a, b in pairs], None,
                             chain.classes, 1.0)
        assert torch.equal(chain.image(gd.auto_normalize), plain[k]), k


def test_sample_and_interpolate_take_classes(case):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    dev = case.dev
    gd = GaussianDiffusion(case.net, img_size=case.S, timesteps=6, objective=case.o, cond_scale=2.0).to(dev)
    y = torch.tensor([1, 4], device=dev)
    torch.manual_seed(4)
    a = gd.sample(batch_size=2, classes=y)                     # cond_scale=None: the constructor's 2.0
    torch.manual_seed(4)
    b = gd.sample(batch_size=2, classes=y, cond_scale=2.0)
    torch.manual_seed(4)
    c = gd.sample(batch_size=2, classes=y, cond_scale=1.0)
    torch.manual_seed(4)
    d = gd.sample(batch_size=2)                                # null labels, one forward
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(c, d) and torch.isfinite(a).all()
    out = gd.sample(batch_size=2, return_all_timesteps=True, classes=y)
    assert out.shape == (2, 7, 3, 16, 16) and torch.isfinite(out).all()
    x1, x2 = torch.rand(2, 3, 16, 16, device=dev) * 2 - 1, torch.rand(2, 3, 16, 16, device=dev) * 2 - 1
    assert torch.isfinite(gd.interpolate(x1, x2, t=4, classes=y, cond_scale=2.0)).all()


# ----------------------------------------------------------------------------------------------------------------------
# the graph-replayed training step with in-graph label drop, optimiser, EMA, checkpoints, train.py
# ----------------------------------------------------------------------------------------------------------------------
def _module(dev, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(img_size=16, dim=16, lr=1e-3, num_classes=5, cond_drop_prob=0.5, ema_update_every=2, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("kw", [dict(), dict(objective="pred_noise", offset_noise_strength=0.1, self_condition=True)],
                         ids=["pred_v", "pred_noise_offset_selfcond"])
def test_graph_replayed_training_step_equals_eager_steps(dev, kw):
    """Four steps through ``make_fast_step`` with the label drop (probability 0.5) drawn on the same seeded device generator:
    losses, parameters after Adam, the EMA shadow and the Adam state of graph replay and eager launches are the same bits."""
    a, b = _module(dev, **kw), _module(dev, **kw)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True), b.make_fast_step(ob, 1, False)
    g = torch.Generator().manual_seed(8)
    coins = [False, True, True, False]
    xs = [torch.rand(8, 3, 16, 16, generator=g).to(dev) for _ in coins]
    ys = [torch.randint(0, 5, (8,), generator=g).to(dev) for _ in coins]
    losses, dropped = {}, 0
    for name, fast in (("graph", fa), ("eager", fb)):
        torch.manual_seed(77)                                  # the device generator: same draws in both runs
        fast.coin = iter(coins).__next__
        losses[name] = []
        for i, (x, y) in enumerate(zip(xs, ys)):
            losses[name].append(fast.step((x.clone(), y.clone()), i).detach().clone().reshape(()))
            if name == "graph":
                used = fast.graphed.classes
                assert bool(((used == y) | (used == 5)).all())
                dropped += int((used != y).sum())
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    assert 0 < dropped < 8 * len(coins), "some labels were dropped inside the graph, not all"
    for la, lb in zip(losses["graph"], losses["eager"]):
        assert torch.isfinite(la) and torch.equal(la, lb), (float(la), float(lb))
    assert len({float(x) for x in losses["graph"]}) == len(coins)
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data)
    assert torch.equal(a.ema.ema_model.model._flat.data, b.ema.ema_model.model._flat.data)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    for pa, pb in zip(oa.state_dict()["state"].values(), ob.state_dict()["state"].values()):
        for k in pb:
            assert torch.equal(torch.as_tensor(pa[k]), torch.as_tensor(pb[k])), k


def test_fused_adam_ema_and_checkpoints(fx, dev, parity):
    """One FusedAdam step on the HIP gradient against torch.optim.Adam on the fixture's (1e-6, the bound of the Adam
    interchange test of tests/test_hip_unet.py); the EMA shadow's embedding has its own storage; state_dict and the optimizer
    checkpoint round-trip."""
    from lgm_hip.optim import EMA, FusedAdam
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    case = _Case(fx, "pred_v", dev)
    net, gd = case.net, case.gd
    ema = EMA(gd, beta=0.995, update_every=1)
    ema.ema_model.model.prepare_hip(dev)
    w_on, w_sh = net.label_emb.weight, ema.ema_model.model.label_emb.weight
    assert w_on.data_ptr() != w_sh.data_ptr() and torch.equal(w_on, w_sh)
    assert net._flat.slot(w_on).offset < net._head_end, "the embedding sits in the FiLM + time bucket"
    opt = FusedAdam(net.parameters(), lr=1e-3, betas=(0.9, 0.99))
    net._flat.zero_grad()
    gd.p_losses((case.img * 2 - 1).to(dev), case.t.to(dev), case.noise.to(dev), classes=case.classes.to(dev)).backward()
    opt.step()
    ref = torch.nn.Parameter(torch.as_tensor(fx["label_emb.weight"]).clone())
    ref.grad = torch.as_tensor(case.fx["grad:label_emb.weight"]).clone()
    torch.optim.Adam([ref], lr=1e-3, betas=(0.9, 0.99)).step()
    parity("label_emb.weight after one FusedAdam step vs torch.optim.Adam on the fixture gradient", rel(w_on, ref), 1e-6)
    assert torch.equal(w_on[[1, 2, 4]].cpu(), torch.as_tensor(fx["label_emb.weight"])[[1, 2, 4]]), "zero gradient: no update"
    assert not torch.equal(w_on, w_sh)
    ema.update()
    assert torch.equal(w_on, w_sh) and w_on.data_ptr() != w_sh.data_ptr()      # the first update copies, into its own storage
    # checkpoints
    x, t, y = case.x_t.to(dev), case.t.to(dev), case.classes.to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    other = Unet(dim=16, channels=3, num_classes=5)
    other.load_state_dict(sd, strict=True)
    GaussianDiffusion(other, img_size=16).to(dev)
    other.prepare_hip(dev)
    with torch.no_grad():
        assert torch.equal(other(x, t, classes=y), net(x, t, classes=y))
    osd = opt.state_dict()
    idx = [n for n, _ in net.named_parameters()].index("label_emb.weight")
    assert tuple(osd["state"][idx]["exp_avg"].shape) == (6, 64)
    opt2 = FusedAdam(other.parameters(), lr=1e-3, betas=(0.9, 0.99))
    opt2.load_state_dict(osd)
    back = opt2.state_dict()
    for i, ent in osd["state"].items():
        for k in ent:
            assert torch.equal(torch.as_tensor(back["state"][i][k]), torch.as_tensor(ent[k])), (i, k)


def test_train_entry_runs_the_cond_config(tmp_path):
    """train.py's main() on configs/diffusion/ddpm_cond.json at a reduced size (16 x 16, dim 16, 20 diffusion steps: the
    step-0 sample is a 20-step guided ancestral chain of 64 images), six steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "ddpm_cond.json")))
    assert cfg["model"]["args"]["num_classes"] == 10 and cfg["model"]["args"]["cond_scale"] == 3.0
    cfg["model"]["args"].update(img_size=16, dim=16, diffusion_timesteps=20)
    cfg["dataset"].update(img_size=16, batch_size=8)
    path = tmp_path / "ddpm_cond_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_ddpm_cond"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('LAST_SAMPLES', tuple(m.last_samples.shape), bool(torch.isfinite(m.last_samples).all())); "
            "print('TRAIN_LOSS', float(m.logged['train_loss']))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "6", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("LAST_SAMPLES", "TRAIN_LOSS"))}
    assert lines["LAST_SAMPLES"] == "LAST_SAMPLES (64, 3, 16, 16) True", lines
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 6 and sd["hyper_parameters"]["num_classes"] == 10
    assert tuple(sd["state_dict"]["ema.online_model.model.label_emb.weight"].shape) == (11, 64)
    for v in sd["state_dict"].values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
