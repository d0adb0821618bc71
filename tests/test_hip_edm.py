"""GPU: elucidated diffusion (``models.generative.diffusion.edm``; Karras et al. 2022; an extension of the reference) and the
random / learned Fourier time embedding of ``Unet``.

  * the kernels of csrc/edm.hip per element against the float64 restatement of tests/edm_ref.py under (k + 2) u M, k =
    ``edm_ref.ROUNDINGS`` (DESIGN 6 derives them): both q_sample forms, pre / euler / heun with the row by value and from a
    table (the same bits), sentinels, lane padding, the clamp acting on some elements and not on others, the Fourier row and
    its weight gradient at B = 1, 4, 128;
  * F, the loss and ALL parameter gradients against the reference's own ``Unet(learned_sinusoidal_cond=True)``
    (tests/golden/diffusion_edm.npz, tools/make_golden_edm.py), 1e-4 relative; random features: the same forward, no gradient,
    the frequencies bit-unchanged by an optimizer step;
  * the four chains of the fixture with injected noises under max(1e-4, 4 x the fixture's float32-to-float64 distance);
  * graph replay bit for bit against eager launches: the training step (plain, accumulating + clipping, class-conditional)
    and every chain with drawn noise; three steps of ``EDM`` against forward + backward + the same optimizer; train.py;
  * the paths that were there before: a sinusoidal DDPM step and a DDIM chain against the bits and the launch trace recorded
    on the commit before (tests/golden/diffusion_edm_unchanged.json); a Fourier step under ``LGM_TIME_MLP=1``; the 16-byte
    stores beside sentinel lanes of a wider input buffer.

Measured distances go through the ``parity`` recorder (committed record: profiles/r21_edm_parity.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edm_ref as ER

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = ER.U
SENTINEL = 7.0
SD = 0.5


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
    return dict(np.load(os.path.join(golden_dir, "diffusion_edm.npz")))


def _r4(n):
    return (n + 3) // 4 * 4


def _nchw(t, C):
    """NHWC device buffer -> float64 numpy NCHW of its first C lanes"""
    return t[..., :C].permute(0, 3, 1, 2).double().cpu().numpy()


def _nhwc(a, pitch, dev):
    """float NCHW numpy / tensor -> NHWC float32 device buffer of ``pitch`` lanes, padding zero"""
    a = torch.as_tensor(a, dtype=torch.float32)
    B, C, H, W = a.shape
    buf = torch.zeros((B, H, W, pitch), device=dev)
    buf[..., :C] = a.permute(0, 2, 3, 1).to(dev)
    return buf


def _within(got, want, mag, k, what, parity):
    """per element |got - want| <= (k + 2) u mag; the worst ratio goes on record"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bound = (k + 2) * U * np.maximum(mag, 1e-300)
    parity(what + f" [worst |err| / ((k + 2) u M), k = {k}]", float((err / bound).max()), 1.0)


SHAPES = [(3, 3, 8, 8), (3, 1, 8, 8), (3, 3, 6, 6), (3, 1, 6, 6), (3, 3, 32, 32)]
IDS = ["3x3x8x8", "3x1x8x8", "3x3x6x6_ragged", "3x1x6x6_ragged", "3x3x32x32_several_workgroups"]


# ----------------------------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True], ids=["normalised", "data_range"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_qsample_against_the_float64_restatement(dev, parity, shape, normalize):
    """Both forms.  sigma in (0.002, 0.5, 80) among the samples of the explicit form; the drawn form's sigma against float64
    exp under the accuracy HIP documents for device expf (HIP Programming Guide, "HIP math API", single precision: expf 1 ULP),
    everything downstream against float64 from the kernel's own float32 sigma; the two forms agree to the bit when the second
    is handed the first one's sigma (c_noise apart, which the explicit form takes through a logarithm)."""
    from lgm_hip import ops
    B, C, H, W = shape
    Cp = _r4(C)
    g = torch.Generator().manual_seed(11)
    img = torch.rand(shape, generator=g) if normalize else torch.randn(shape, generator=g)
    eps = torch.randn(shape, generator=g)
    n = torch.tensor([-1.3, 0.4, 2.1])
    P_mean, P_std = -1.2, 1.2
    out = {}
    for form, kw in (("sigma", dict(sigma=torch.tensor([0.002, 0.5, 80.0]).to(dev))),
                     ("n", dict(n=n.to(dev), P_mean=P_mean, P_std=P_std))):
        xin = torch.full((B, H, W, Cp), SENTINEL, device=dev)
        flat = torch.full((B * H * W * Cp + 128,), SENTINEL, device=dev)
        target = flat[64:-64].view(B, H, W, Cp)
        sig, cn = torch.full((B,), SENTINEL, device=dev), torch.full((B,), SENTINEL, device=dev)
        ops.edm_qsample(img.to(dev), eps.to(dev), xin, 0, target, sig, cn, SD, normalize, **kw)
        torch.cuda.synchronize()
        assert bool((flat[:64] == SENTINEL).all()) and bool((flat[-64:] == SENTINEL).all()), "nothing outside the target"
        assert bool((xin[..., C:] == 0).all()) and bool((target[..., C:] == 0).all()), "padding as lgm_qsample_target_slice leaves it"
        s32 = sig.double().cpu().numpy()
        if form == "sigma":
            assert s32.tolist() == [float(np.float32(v)) for v in (0.002, 0.5, 80.0)]
            want_cn = np.log(s32) / 4
            cn_tol = 2.0 ** -23 * np.abs(np.log(s32)) / 4 * (1 + 1e-9)          # logf: 1 ULP (same table); the quarter is exact
        else:
            ls = (np.float32(P_mean) + (np.float32(P_std) * n.numpy()).astype(np.float32)).astype(np.float32).astype(np.float64)
            assert np.all(np.abs(s32 - np.exp(ls)) <= 2.0 ** -23 * np.exp(ls)), "expf within 1 ULP of exp(float32 ln sigma)"
            want_cn, cn_tol = ls / 4, 0.0
            assert np.all(s32 > 0) and len(set(s32.tolist())) == B
        assert np.all(np.abs(cn.double().cpu().numpy() - want_cn) <= cn_tol), (form, cn.tolist(), want_cn)
        y = img.double().numpy() * 2 - 1 if normalize else img.double().numpy()
        _, want_x, want_t, mx, mt = ER.qsample(y, eps.double().numpy(), s32, SD)
        _within(_nchw(xin, C), want_x, mx, ER.ROUNDINGS["xin"], f"edm_qsample[{form}] c_in x", parity)
        _within(_nchw(target, C), want_t, mt, ER.ROUNDINGS["target"], f"edm_qsample[{form}] F*", parity)
        out[form] = (xin, target, sig)
    # the drawn form's sigma handed to the explicit form: the same bits
    xin2, target2 = torch.zeros_like(out["n"][0]), torch.zeros_like(out["n"][1])
    sig2, cn2 = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    ops.edm_qsample(img.to(dev), eps.to(dev), xin2, 0, target2, sig2, cn2, SD, normalize, sigma=out["n"][2].clone())
    assert torch.equal(xin2, out["n"][0]) and torch.equal(target2, out["n"][1]) and torch.equal(sig2, out["n"][2])


def test_qsample_scalar_access_form_gives_the_same_bits(dev):
    """an input buffer whose x slice starts at an odd lane takes one lane per thread: the bits of the 16-byte form"""
    from lgm_hip import ops
    B, C, H, W = 3, 3, 6, 6
    g = torch.Generator().manual_seed(12)
    img, eps = torch.randn(B, C, H, W, generator=g).to(dev), torch.randn(B, C, H, W, generator=g).to(dev)
    sigma = torch.tensor([0.002, 0.5, 80.0]).to(dev)
    a, ta = torch.zeros((B, H, W, 4), device=dev), torch.zeros((B, H, W, 4), device=dev)
    b, tb = torch.full((B, H, W, 8), SENTINEL, device=dev), torch.zeros((B, H, W, 4), device=dev)
    s, c = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    ops.edm_qsample(img, eps, a, 0, ta, s, c, SD, False, sigma=sigma)
    ops.edm_qsample(img, eps, b, 3, tb, s, c, SD, False, sigma=sigma)
    assert torch.equal(b[..., 3:6], a[..., :3]) and torch.equal(ta, tb)
    assert bool((b[..., :3] == SENTINEL).all()) and bool((b[..., 7:] == SENTINEL).all()) and bool((b[..., 6] == 0).all())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sampling_kernels_against_the_float64_restatement(dev, parity, shape):
    """pre -> euler -> heun of one churned step and one last step, the row by value and from a table: every output per element
    under its bound, from the kernel's own float32 inputs; the two row forms agree to the bit; the clamp acts on some elements
    and not on others; the table's other rows, the counter's neighbours and the buffers of a step without a second evaluation
    keep their sentinels."""
    from lgm_hip import ops
    B, C, H, W = shape
    Cp = _r4(C)
    rows64 = ER.plan(6, 0.002, 80.0, SD, 7.0, churn=1.8)
    table = torch.full((8, 16), SENTINEL, device=dev)
    table[2] = torch.tensor(rows64[3], dtype=torch.float32)           # sigma 0.97 -> 0.085, gamma 0.3
    table[3] = torch.tensor(rows64[5], dtype=torch.float32)           # the last step: sigma 0.002 -> 0
    g = torch.Generator().manual_seed(13)
    for r, second in ((2, True), (3, False)):
        row = table[r].double().cpu().numpy()                          # the float32 row the kernels read, as float64
        scale = float(row[1])
        x = torch.randn(shape, generator=g) * max(scale, 0.6) * 1.5 + 0.3      # (the last step: D is about x, clamped where |x| > 1)
        eps = torch.randn(shape, generator=g)
        F1, F2 = torch.randn(shape, generator=g) * 1.5, torch.randn(shape, generator=g) * 1.5
        res = {}
        for form in ("value", "table"):
            counter = torch.tensor([7, r, 7], dtype=torch.int32, device=dev)
            kw = dict(row=table[r].tolist()) if form == "value" else dict(table=table, counter=counter[1:2])
            adv = form == "table"
            st = {k: torch.full((B, H, W, Cp), SENTINEL, device=dev) for k in ("xhat", "d", "xin")}
            xs = _nhwc(x, Cp, dev)
            cn = torch.full((B,), SENTINEL, device=dev)
            ops.edm_pre(xs, eps.to(dev), st["xhat"], st["xin"], 0, cn, C, **kw)
            xin1, cn1 = st["xin"].clone(), cn.clone()
            ops.edm_euler(_nhwc(F1, Cp, dev), st["xhat"], xs, C, True, d=st["d"] if second else None,
                          xin=st["xin"] if second else None, cnoise=cn if second else None, second=second,
                          advance=adv and not second, **kw)
            xp = xs.clone()
            if second:
                ops.edm_heun(_nhwc(F2, Cp, dev), st["xhat"], st["d"], xs, C, True, advance=adv, **kw)
            torch.cuda.synchronize()
            res[form] = dict(xhat=st["xhat"], xin1=xin1, cn1=cn1, xp=xp, d=st["d"], xin2=st["xin"], cn2=cn, x=xs)
            if form == "table":
                assert counter.tolist() == [7, r + 1, 7], "the step's last launch advances the counter, and nothing else"
        assert bool((table[[0, 1, 4, 5, 6, 7]] == SENTINEL).all())
        for k in res["value"]:
            assert torch.equal(res["value"][k], res["table"][k]), (k, "row by value and from the table: the same bits")
        v = res["value"]
        for k in ("xhat", "xin1", "xp", "x") + (("d", "xin2") if second else ()):
            assert bool((v[k][..., C:] == 0).all()), (k, "padding lanes are zero")
        if not second:
            assert bool((v["d"] == SENTINEL).all()) and torch.equal(v["xin2"], v["xin1"]) and torch.equal(v["cn2"], v["cn1"])
        x64, e64 = x.double().numpy(), eps.double().numpy()
        xh, xin, mh, mi = ER.pre(x64, e64, row)
        _within(_nchw(v["xhat"], C), xh, mh, ER.ROUNDINGS["xhat"], f"edm_pre x^ (second={second})", parity)
        _within(_nchw(v["xin1"], C), xin, mi, ER.ROUNDINGS["pre_xin"], f"edm_pre c_in x^ (second={second})", parity)
        assert v["cn1"].tolist() == [float(np.float32(row[5]))] * B
        assert (not second) or not np.array_equal(_nchw(v["xhat"], C), x.double().numpy()), "a churned step adds its noise"
        if not second:
            assert torch.equal(v["xhat"], _nhwc(x, Cp, dev)), "no churn on the last step: x^ is x, bit for bit"
        # downstream from the kernel's own x^
        xh32 = _nchw(v["xhat"], C)
        xp64, d64, xin2, raw, mxp, md = ER.euler(xh32, F1.double().numpy(), row, True)
        acted = np.abs(raw) > 1
        assert acted.any() and not acted.all(), "the clamp acts on some elements and not on others"
        _within(_nchw(v["xp"], C), xp64, mxp, ER.ROUNDINGS["euler_x"], f"edm_euler x' (second={second})", parity)
        if second:
            _within(_nchw(v["d"], C), d64, md, ER.ROUNDINGS["euler_d"], "edm_euler d", parity)
            _within(_nchw(v["xin2"], C), xin2, row[8] * mxp, ER.ROUNDINGS["euler_xin"], "edm_euler c_in' x'", parity)
            assert v["cn2"].tolist() == [float(np.float32(row[9]))] * B
            xn, raw2, mn = ER.heun(xh32, _nchw(v["xp"], C), _nchw(v["d"], C), F2.double().numpy(), row, True)
            acted2 = np.abs(raw2) > 1
            assert acted2.any() and not acted2.all()
            _within(_nchw(v["x"], C), xn, mn, ER.ROUNDINGS["heun_x"], "edm_heun x_next", parity)


@pytest.mark.parametrize("B", [1, 4, 128])
def test_fourier_embedding_forward_and_backward(dev, parity, B):
    """the row (x, sin, cos) at the padded pitch and the weight gradient against float64 from the kernel's own float32
    operands; the backward has equal bits across two runs and honours beta"""
    from lgm_hip import ops
    half, pitch = 8, 20
    g = torch.Generator().manual_seed(14 + B)
    x = (torch.randn(B, generator=g) * 0.6 - 0.3).to(dev)               # c_noise = ln(sigma) / 4 lies in about [-1.6, 1.1]
    w = torch.randn(half, generator=g).to(dev)
    out = torch.full((B, pitch), SENTINEL, device=dev)
    ops.fourier_emb_fwd(x, w.data_ptr(), half, out)
    want, mag = ER.fourier_row(x.double().cpu().numpy(), w.double().cpu().numpy())
    got = out.double().cpu().numpy()
    assert np.array_equal(got[:, 0], x.double().cpu().numpy()) and np.all(got[:, 2 * half + 1:] == 0)
    _within(got[:, :2 * half + 1], want, mag, ER.ROUNDINGS["fourier"], f"fourier_emb_fwd B={B}", parity)
    gemb = torch.randn(B, pitch, generator=g).to(dev)
    gw = [torch.full((half + 4,), SENTINEL, device=dev) for _ in range(3)]
    ops.fourier_emb_bwd(out, gemb, half, gw[0].data_ptr(), 0.0)
    ops.fourier_emb_bwd(out, gemb, half, gw[1].data_ptr(), 0.0)
    gw[2][:half] = 2.0
    ops.fourier_emb_bwd(out, gemb, half, gw[2].data_ptr(), 1.0)
    torch.cuda.synchronize()
    assert torch.equal(gw[0], gw[1]), "no atomics: the same bits on every run"
    assert bool((gw[0][half:] == SENTINEL).all())
    wg, mg = ER.fourier_wgrad(got, gemb.double().cpu().numpy(), half)
    _within(gw[0][:half].double().cpu().numpy(), wg, mg, B + 4, f"fourier_emb_bwd B={B}", parity)
    assert torch.equal(gw[2][:half], (gw[0][:half] + 2.0)), "beta = 1 accumulates"


# ----------------------------------------------------------------------------------------------------------------------
# the network against the reference's own
# ----------------------------------------------------------------------------------------------------------------------
def _weights(fx):
    from oracle import diffusion as OD
    P = dict(OD.unet_init(dim=int(fx["dim"]), channels=3, seed=int(fx["seed"])))
    for k in ("time_mlp.0.weights", "time_mlp.1.weight", "time_mlp.1.bias"):
        P[k] = torch.as_tensor(fx[k])
    return P


def _diffusion(fx, dev, random=False, classes=False, **kw):
    from models.generative.diffusion.ddpm import Unet
    from models.generative.diffusion.edm import ElucidatedDiffusion
    four = dict(random_fourier_features=True) if random else dict(learned_sinusoidal_cond=True)
    net = Unet(dim=int(fx["dim"]), channels=3, num_classes=int(fx["K"]) if classes else None, **four)
    P = _weights(fx)
    if classes:
        P["label_emb.weight"] = torch.as_tensor(fx["label_emb.weight"])
    net.load_state_dict(P, strict=True)
    ed = ElucidatedDiffusion(net, img_size=int(fx["S"]), **kw).to(dev)
    net.prepare_hip(dev)
    return ed


def _data(fx, dev):
    B, S = int(fx["B"]), int(fx["S"])
    g = torch.Generator().manual_seed(int(fx["data_seed"]))
    img = torch.rand(B, 3, S, S, generator=g).to(dev)
    noise = torch.randn(B, 3, S, S, generator=g).to(dev)
    return img, noise, torch.as_tensor(fx["sigma"], dtype=torch.float32).to(dev)


def test_network_loss_and_all_gradients_match_the_reference_fixture(fx, dev, parity):
    from models.generative.diffusion.edm import edm_loss_qsample
    ed = _diffusion(fx, dev)
    net = ed.model
    img, noise, sigma = _data(fx, dev)
    c = {k[len("learned:"):]: v for k, v in fx.items() if k.startswith("learned:")}
    q = edm_loss_qsample(ed, img, noise, True, sigma=sigma)
    F, _ = net.forward_nhwc(q.xt, q.net_t, False)
    F = F[..., :3].permute(0, 3, 1, 2)
    parity.record("F [distances to float64]", hip_vs_ref=rel(F, c["F"]), ref_vs_fp64=rel(c["F"], c["F64"]),
                  hip_vs_fp64=rel(F, c["F64"]))
    parity("F at explicit (x, sigma)", rel(F, c["F"]), RTOL)
    x = torch.as_tensor(fx["x"]).to(dev)
    c_in = (1.0 / torch.sqrt(sigma.double() ** 2 + SD ** 2)).float().view(-1, 1, 1, 1)
    with torch.no_grad():
        parity("Unet.forward(c_in x, c_noise), NCHW", rel(net(x * c_in, torch.log(sigma) / 4), c["F"]), RTOL)
    D = ed.preconditioned(x, sigma)
    _, _, c_skip, c_out = (torch.as_tensor(ER.col(v)) for v in ER.coefficients(fx["sigma"], SD))
    parity("preconditioned D", rel(D, c_skip * torch.as_tensor(fx["x"]).double() + c_out * torch.as_tensor(c["F64"])), RTOL)
    net._flat.zero_grad()
    loss = ed.p_losses(img, sigma, noise, _normalize=True)
    want = float(c["loss"])
    parity.record("loss [distances to float64]", hip_vs_ref=abs(loss.item() - want) / want,
                  ref_vs_fp64=abs(want - float(c["loss64"])) / float(c["loss64"]),
                  hip_vs_fp64=abs(loss.item() - float(c["loss64"])) / float(c["loss64"]))
    parity("loss (F-space MSE against the reference's textbook form)", abs(loss.item() - want) / want, RTOL)
    loss.backward()
    sd = dict(net.named_parameters())
    worst, worst_n, worst_s, seen, Ks = 0.0, 0.0, 0.0, set(), int(fx["grad_sample"])
    for k in c:
        if k.startswith("grad:"):
            worst = max(worst, rel(sd[k[5:]].grad, c[k]))
            seen.add(k[5:])
        elif k.startswith("gradnorm:"):
            n = k[9:]
            worst_n = max(worst_n, abs(sd[n].grad.double().norm().item() - float(c[k])) / max(float(c[k]), 1e-12))
            flat = sd[n].grad.reshape(-1)
            worst_s = max(worst_s, rel(flat[:: flat.numel() // Ks][:Ks], c["gradsample:" + n]))
            seen.add(n)
    assert seen == set(sd) and "time_mlp.0.weights" in seen, "ALL parameters are in the fixture, the frequencies included"
    parity("gradient of time_mlp.0.weights", rel(sd["time_mlp.0.weights"].grad, c["grad:time_mlp.0.weights"]), RTOL)
    parity("worst parameter gradient (whole tensors)", worst, RTOL)
    parity("worst gradient norm (large tensors)", worst_n, RTOL)
    parity(f"worst {Ks}-element gradient sample (large tensors)", worst_s, RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    parity("all-parameter gradient norm", abs(gn - float(c["gradnorm_all"])) / float(c["gradnorm_all"]), RTOL)
    net._flat.zero_grad()


def test_random_features_same_forward_no_gradient_and_untouched_by_the_optimizer(fx, dev, parity):
    from lgm_hip.optim import FusedAdam
    ed = _diffusion(fx, dev, random=True)
    net = ed.model
    img, noise, sigma = _data(fx, dev)
    w = net.time_mlp[0].weights
    before = w.detach().clone()
    others = net.time_mlp[1].weight.detach().clone()
    opt = FusedAdam(ed.parameters(), lr=1e-2)
    loss = ed.p_losses(img, sigma, noise, _normalize=True)
    parity("random features: loss", abs(loss.item() - float(fx["random:loss"])) / float(fx["random:loss"]), RTOL)
    loss.backward()
    slot = net._flat.slot(w)
    assert bool((net._flat.grad[slot.offset:slot.offset + slot.numel] == 0).all()), "no gradient for the frequencies"
    parity("random features: gradient of time_mlp.1.bias", rel(net.time_mlp[1].bias.grad, fx["random:grad:time_mlp.1.bias"]), RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters() if p.grad is not None)).item()
    parity("random features: all-parameter gradient norm", abs(gn - float(fx["random:gradnorm_all"])) / float(fx["random:gradnorm_all"]),
           RTOL)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(w.detach(), before), "the optimizer leaves the random features bit-unchanged"
    assert not torch.equal(net.time_mlp[1].weight.detach(), others), "and moves everything else"


# ----------------------------------------------------------------------------------------------------------------------
# chains
# ----------------------------------------------------------------------------------------------------------------------
def _chain_setup(fx, dev, name):
    kind, N, churn, guided = fx[f"{name}:spec"]
    N, churn, guided = int(N), float(churn), bool(int(guided))
    ed = _diffusion(fx, dev, classes=guided, num_sample_steps=N, S_churn=churn)
    ed.eval()
    kw = dict(sampler=str(kind))
    if guided:
        kw.update(classes=torch.as_tensor(fx["guided_classes"]).to(dev), cond_scale=float(fx["guided_scale"]))
    return ed, N, churn, kw


@pytest.mark.parametrize("name", ["heun8", "euler8", "churn6", "guided4"])
def test_chains_match_the_reference_fixture(fx, dev, parity, name, monkeypatch):
    """injected noises; bound max(1e-4, 4 x the fixture's own float32-to-float64 distance), relative to max |image|; graph
    replay and eager launches give the same bits"""
    ed, N, churn, kw = _chain_setup(fx, dev, name)
    init = torch.as_tensor(fx[f"{name}:init"]).to(dev)
    noises = [torch.as_tensor(v).to(dev) for v in fx[f"{name}:noises"]] if churn > 0 else None
    got = ed.sample(batch_size=int(fx["B"]), init_noise=init, noises=noises, **kw)
    ref, ref64 = torch.as_tensor(fx[f"{name}:image"]).double(), torch.as_tensor(fx[f"{name}:image64"])
    dist = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())  # noqa: E731
    bound = max(1e-4, 4 * float(fx[f"{name}:dist"]))
    parity.record(f"{name} [distances relative to max |image|]", hip_vs_ref=dist(got, ref), ref_vs_fp64=float(fx[f"{name}:dist"]),
                  hip_vs_fp64=dist(got, ref64), bound=bound)
    parity(f"{name}: final image against float64", dist(got, ref64), bound)
    parity(f"{name}: final image against the reference's float32", dist(got, ref), 2 * bound)
    from lgm_hip import captured
    keys = [k for k in captured._GRAPHS.get(ed.model, {}) if k[0] == "edm"]
    assert len(keys) == (2 if kw["sampler"] == "heun" else 1), keys
    assert all(not isinstance(v, int) for v in captured._GRAPHS[ed.model].values()), "the steps were captured"
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = ed.sample(batch_size=int(fx["B"]), init_noise=init, noises=noises, **kw)
    assert torch.equal(got, eager), "graph replay and eager launches: the same bits"
    every = ed.sample(batch_size=int(fx["B"]), init_noise=init, noises=noises, return_all_timesteps=True, **kw)
    assert tuple(every.shape) == (int(fx["B"]), N + 1, 3, int(fx["S"]), int(fx["S"])) and torch.equal(every[:, -1], got)


@pytest.mark.parametrize("name", ["heun8", "euler8", "churn6", "guided4"])
def test_chains_with_drawn_noise_graph_replay_equals_eager(fx, dev, name, monkeypatch):
    ed, N, churn, kw = _chain_setup(fx, dev, name)
    B = int(fx["B"])
    torch.manual_seed(31)
    a = ed.sample(batch_size=B, **kw)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    torch.manual_seed(31)
    b = ed.sample(batch_size=B, **kw)
    torch.manual_seed(32)
    c = ed.sample(batch_size=B, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and bool(torch.isfinite(a).all())


# ----------------------------------------------------------------------------------------------------------------------
# training
# ----------------------------------------------------------------------------------------------------------------------
def _module(dev, **kw):
    from models.generative.diffusion.edm import EDM
    torch.manual_seed(10)
    m = EDM(**dict(dict(img_size=16, dim=16, lr=1e-3, ema_update_every=2), **kw))
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("kw,acc,clip", [(dict(), 1, None), (dict(), 2, 0.5), (dict(num_classes=3), 1, None),
                                         (dict(random_fourier_features=True, learned_sinusoidal_cond=False, dropout=0.1), 1, None)],
                         ids=["plain_step", "accumulate2_clipped", "class_conditional", "random_features_dropout"])
def test_graph_replayed_training_step_equals_eager_steps(dev, kw, acc, clip):
    """Four steps through ``make_fast_step``: losses, parameters after Adam, the EMA shadow and the Adam state of graph replay
    and eager launches are the same bits; two replays draw different sigmas."""
    a, b = _module(dev, **kw), _module(dev, **kw)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    oa.max_grad_norm = ob.max_grad_norm = clip
    fa, fb = a.make_fast_step(oa, 1, True, accumulate=acc), b.make_fast_step(ob, 1, False, accumulate=acc)
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(8, 3, 16, 16, generator=g).to(dev) for _ in range(4)]
    y = (torch.arange(8) % 3).to(dev)
    losses, drawn = {}, []
    for name, fast in (("graph", fa), ("eager", fb)):
        torch.manual_seed(77)
        losses[name] = []
        for i, x in enumerate(xs):
            losses[name].append(fast.step((x.clone(), y), i).detach().clone().reshape(()))
            if name == "graph":
                drawn.append(fast.graphed.t.clone())
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    for la, lb in zip(losses["graph"], losses["eager"]):
        assert torch.isfinite(la) and torch.equal(la, lb), (float(la), float(lb))
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (8,) for t in drawn) and len({tuple(t.tolist()) for t in drawn}) == 4
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data)
    assert torch.equal(a.ema.ema_model.model._flat.data, b.ema.ema_model.model._flat.data)
    w0 = _module(dev, **kw).ema.online_model.model
    assert not torch.equal(na._flat.data, w0._flat.data), "the model trains"
    same = torch.equal(na.time_mlp[0].weights, w0.time_mlp[0].weights)
    assert same == bool(kw.get("random_fourier_features", False)), "learned frequencies train, random ones never move"
    for pa, pb in zip(oa.state_dict()["state"].values(), ob.state_dict()["state"].values()):
        for k in pb:
            assert torch.equal(torch.as_tensor(pa[k]), torch.as_tensor(pb[k])), k


def test_three_steps_of_the_module_equal_forward_backward_and_the_same_optimizer(dev):
    a, b = _module(dev), _module(dev)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa = a.make_fast_step(oa, 1, True)
    g = torch.Generator().manual_seed(9)
    xs = [torch.rand(8, 3, 16, 16, generator=g).to(dev) for _ in range(3)]
    torch.manual_seed(78)
    la = [fa.step((x.clone(), None), i).detach().clone().reshape(()) for i, x in enumerate(xs)]
    torch.manual_seed(78)
    ed, lb = b.ema.online_model, []
    for i, x in enumerate(xs):
        loss = ed(x)
        loss.backward()
        ob.step()
        ob.zero_grad()
        b.on_train_batch_end(None, None, i)
        lb.append(loss.detach().clone().reshape(()))
    assert all(torch.equal(p, q) for p, q in zip(la, lb)), (la, lb)
    assert torch.equal(a.ema.online_model.model._flat.data, ed.model._flat.data)
    assert torch.equal(a.ema.ema_model.model._flat.data, b.ema.ema_model.model._flat.data)
    # the state dict goes round with the reference's keys
    sd = {k: v.detach().cpu().clone() for k, v in ed.model.state_dict().items()}
    from models.generative.diffusion.ddpm import Unet
    fresh = Unet(dim=16, learned_sinusoidal_cond=True)
    fresh.load_state_dict(sd, strict=True)
    fresh.prepare_hip(dev)
    x = torch.randn(2, 3, 16, 16, device=dev)
    t = torch.tensor([-0.7, 0.4], device=dev)
    with torch.no_grad():
        assert torch.equal(fresh(x, t), ed.model(x, t))
    out = a.sample(batch_size=2, steps=3)
    assert tuple(out.shape) == (2, 3, 16, 16) and bool(torch.isfinite(out).all())


def test_train_entry_trains_and_resumes(tmp_path):
    """train.py's main() on configs/diffusion/edm.json at a reduced size (8 x 8, dim 16, 4 sampling steps): a few steps, a
    sample at step 0, then a resume from the checkpoint"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "edm.json")))
    cfg["model"]["args"].update(img_size=8, dim=16, num_sample_steps=4)
    cfg["dataset"].update(img_size=8, batch_size=8)
    path = tmp_path / "edm_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_edm"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('STEPS', m.global_step, m.trainer.fast.mode); print('TRAIN_LOSS', float(m.logged['train_loss'])); "
            "s = m.last_samples; print('SAMPLES', None if s is None else (tuple(s.shape), bool(torch.isfinite(s).all())))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "5", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "TRAIN_LOSS", "SAMPLES"))}
    assert lines["STEPS"].startswith("STEPS 5 hipGraph replay"), lines
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    assert lines["SAMPLES"] == "SAMPLES ((64, 3, 8, 8), True)", lines            # the sample logged at step 0
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 5 and sd["hyper_parameters"]["num_sample_steps"] == 4
    assert "ema.online_model.model.time_mlp.0.weights" in sd["state_dict"] and "ema.ema_model.model.time_mlp.0.weights" in sd["state_dict"]
    for v in sd["state_dict"].values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
    r = subprocess.run(cmd[:-4] + ["--max_steps", "8", "--experiment_name", exp, "--ckpt_path", ck], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "STEPS 8 hipGraph replay" in r.stdout and "SAMPLES None" in r.stdout      # (steps 5 .. 7 log no sample)
    assert torch.load(ck, map_location="cpu", weights_only=False)["global_step"] == 8


# ----------------------------------------------------------------------------------------------------------------------
# the paths that were there before
# ----------------------------------------------------------------------------------------------------------------------
def test_sinusoidal_step_and_ddim_chain_give_the_bits_and_the_launch_trace_they_gave(dev, golden_dir):
    """A sinusoidal ``DDPM`` - one eager training step, two graph-replayed ones, a DDIM chain eager and replayed - against
    tests/golden/diffusion_edm_unchanged.json, recorded by tools/make_golden_edm_unchanged.py on a checkout of the commit
    before the Fourier embedding (tests/edm_unchanged.py is the run on both sides): the same entry points in the same order,
    the same loss, gradient, parameter, shadow and image bits."""
    import edm_unchanged
    want = json.load(open(os.path.join(golden_dir, "diffusion_edm_unchanged.json")))
    got = edm_unchanged.measure(dev)
    for part in ("step", "ddim"):
        assert got[part]["trace"] == want[part]["trace"], (part, "the launch trace changed")
        assert not any("edm" in n or "fourier" in n for n in got[part]["trace"])
    assert len(want["step"]["trace"]) > 100 and len(want["ddim"]["trace"]) > 100
    assert got["graph_steps"]["mode"].startswith("hipGraph")
    assert got == want
    assert got["ddim"]["image"] == got["ddim"]["image_graph_replay"]


def test_fourier_network_never_takes_the_fused_sinusoidal_time_mlp(fx, dev, monkeypatch):
    """``LGM_TIME_MLP=1`` (the opt-in fused sinusoidal kernels): a Fourier network stays on the unfused path in the forward
    AND the backward - the loss and every gradient, the frequencies' included, are the bits of a run without the switch."""
    from lgm_hip import ops
    img, noise, sigma = _data(fx, dev)

    def run():
        ed = _diffusion(fx, dev)
        loss = ed.p_losses(img, sigma, noise, _normalize=True)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), ed.model._flat.grad.clone(), ed.model
    l0, g0, _ = run()
    monkeypatch.setattr(ops, "TIME_MLP", True)
    ops._TIME_MLP_OK.clear()
    try:
        plain = _diffusion(fx, dev).model
        from models.generative.diffusion.ddpm import Unet
        assert ops.time_mlp_ok(16, 64, plain.time_mlp[1], plain.time_mlp[3]), "the switch is on for these widths"
        assert Unet(dim=16)._time_mlp_fused() and not plain._time_mlp_fused()
        l1, g1, net = run()
    finally:
        ops._TIME_MLP_OK.clear()
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    w = net._flat.slot(net.time_mlp[0].weights)
    assert bool((g1[w.offset:w.offset + 8] != 0).all()), "the frequencies got their gradient"


def test_vector_stores_leave_the_neighbouring_lanes_of_a_wider_input_buffer_alone(dev):
    """the 16-byte path with the x slice at lane 4 of a pitch of 12: lanes [0, 4) and [8, 12) keep their sentinels in
    ``lgm_edm_qsample``, ``lgm_edm_pre`` and ``lgm_edm_euler``, and lanes [4, 8) hold the bits of the plain layout"""
    from lgm_hip import ops
    B, C, H, W = 3, 3, 6, 6
    g = torch.Generator().manual_seed(15)
    img, eps = torch.randn(B, C, H, W, generator=g).to(dev), torch.randn(B, C, H, W, generator=g).to(dev)
    F = torch.randn(B, H, W, 4, generator=g).to(dev)
    sigma = torch.tensor([0.002, 0.5, 80.0]).to(dev)
    row = ER.plan(6, 0.002, 80.0, SD, 7.0, churn=1.8)[3]
    res = {}
    for name, pitch, off in (("plain", 4, 0), ("wide", 12, 4)):
        q, t = torch.full((B, H, W, pitch), SENTINEL, device=dev), torch.zeros((B, H, W, 4), device=dev)
        s, c = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
        ops.edm_qsample(img, eps, q, off, t, s, c, SD, False, sigma=sigma)
        x = _nhwc(img.cpu(), 4, dev)
        xhat, d = torch.zeros_like(x), torch.zeros_like(x)
        p = torch.full((B, H, W, pitch), SENTINEL, device=dev)
        ops.edm_pre(x, eps, xhat, p, off, c, C, row=row)
        e = torch.full((B, H, W, pitch), SENTINEL, device=dev)
        ops.edm_euler(F, xhat, x, C, True, d=d, xin=e, x_off=off, cnoise=c, second=True, row=row)
        torch.cuda.synchronize()
        res[name] = (q, p, e)
    for plain, wide in zip(res["plain"], res["wide"]):
        assert torch.equal(wide[..., 4:8], plain) and bool((wide[..., :4] == SENTINEL).all()) and bool((wide[..., 8:] == SENTINEL).all())
