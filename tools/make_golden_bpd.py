"""Generate tests/golden/diffusion_bpd.npz: the terms of the variational bound in bits per dimension (Ho et al. 2020 eq. 5;
Nichol & Dhariwal 2021, ``calc_bpd_loop``) around the REAL reference's ``Unet``, ``q_sample``, ``q_posterior`` and
``model_predictions`` on CPU.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_inpaint.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_bpd.py [--check]

The reference has no likelihood evaluation.  The loop of this file is written from the formulas, in their textbook form and
not imported from lgm_hip: per timestep t with the draw eps,
    x_t = q_sample(x0, t, eps);  (eps_pred, x0_pred) = model_predictions(x_t, t, clip_x_start=clip, rederive_pred_noise=True)
    (true_mean, _, lv_q) = q_posterior(x0, x_t, t);  model_mean = q_posterior(x0_pred, x_t, t)[0]
    t >= 1:  mean(0.5 (-1 + lv_p - lv_q + exp(lv_q - lv_p) + (true_mean - model_mean)^2 exp(-lv_p))) / ln 2
    t == 0:  -mean(discretised Gaussian log-likelihood of x0 under (model_mean, 0.5 lv_p)) / ln 2, the tanh CDF and the 1e-12
             floors of Nichol & Dhariwal
    prior:   mean(0.5 (-1 - log(1 - acp_{T-1}) + (1 - acp_{T-1}) + acp_{T-1} x0^2)) / ln 2
with the model's log-variance lv_p = log beta~_t ("small") or log beta_t ("large"), both log beta~_1 at t = 0.  Beside every
term: mean (x0_pred - x0)^2 and mean (eps_pred - eps)^2.

The recipe is the "small" network (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16, B = 4) on 8-bit-quantised uniform
images ("img", seed IMG_SEED).  Cases (the key's first part): pred_v / pred_noise with both variances and clipping
("<objective>:<small|large>"), pred_v small without clipping ("pred_v:noclip"), the self-conditioned network of
tools/make_golden_selfcond.py with a zero self-conditioning input ("pred_v:selfcond") and the label-embedding wrapper of
tools/make_golden_classcond.py with its labels at scale 1 ("pred_v:labels").  Every case on a T = 1000 diffusion at TIMES
("<case>:1000:...") and on a timesteps=20 diffusion in full ("<case>:20:...", with "total").  Draws:
oracle.diffusion.draw_loop_noise(seed, shape, n)[1][i] for the i-th evaluated timestep.  Every result in float32 (the
reference's dtype; key as above) and in float64 (key + "64", from the float64 network and schedule).

Asserted at generation time, in float64: total = sum vb + prior; KC = 0 for every "small" KL row; every decoder term is
finite; the float32 and float64 evaluations of every KL term agree to 1e-3.
"""
from __future__ import annotations

import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_bpd.npz")

from tools.make_golden_classcond import CLASSES, EMB_SEED, K, _Guided, _TimePlusLabel  # noqa: E402
from tools.make_golden_selfcond import INIT_W_SEED, _init_weight  # noqa: E402

T, SHORT_T = 1000, 20
TIMES = (999, 998, 750, 500, 250, 2, 1, 0)
IMG_SEED = 9500
# (case, objective, variance, clip, network extras)
CASES = [("pred_v:small", "pred_v", "small", True, {}), ("pred_v:large", "pred_v", "large", True, {}),
         ("pred_noise:small", "pred_noise", "small", True, {}), ("pred_noise:large", "pred_noise", "large", True, {}),
         ("pred_v:noclip", "pred_v", "small", False, {}),
         ("pred_v:selfcond", "pred_v", "small", True, dict(self_condition=True)),
         ("pred_v:labels", "pred_v", "small", True, dict(labels=True))]
SEEDS = {c[0]: 9501 + i for i, c in enumerate(CASES)}


def approx_cdf(z):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def decoder_ll(x, mean, log_scale):
    """Nichol & Dhariwal's discretized_gaussian_log_likelihood"""
    centered = x - mean
    inv = torch.exp(-log_scale)
    cdf_plus = approx_cdf(inv * (centered + 1.0 / 255.0))
    cdf_min = approx_cdf(inv * (centered - 1.0 / 255.0))
    log_plus = torch.log(cdf_plus.clamp(min=1e-12))
    log_one_minus = torch.log((1.0 - cdf_min).clamp(min=1e-12))
    log_delta = torch.log((cdf_plus - cdf_min).clamp(min=1e-12))
    return torch.where(x < -0.999, log_plus, torch.where(x > 0.999, log_one_minus, log_delta))


def model_logvar(gd, variance):
    lv = gd.posterior_log_variance_clipped
    rest = lv[1:] if variance == "small" else torch.log(gd.betas[1:])
    return torch.cat([lv[1:2], rest])


def flat_mean(x):
    return x.flatten(1).mean(1)


def bpd_terms(gd, x0, times, nz, variance, clip):
    """-> dict of [n, B] / [B] tensors in gd's dtype; also the KC of every KL row (a float per row)"""
    dtype = gd.betas.dtype
    lvp_table = model_logvar(gd, variance)
    ln2 = math.log(2.0)
    vb, xs_mse, mse, kcs = [], [], [], []
    for i, t in enumerate(times):
        tb = torch.full((x0.shape[0],), t, dtype=torch.long)
        eps = nz[i].to(dtype)
        xt = gd.q_sample(x0, tb, eps)
        pred = gd.model_predictions(xt, tb, None, clip_x_start=clip, rederive_pred_noise=True)
        true_mean, _, lv_q = gd.q_posterior(x_start=x0, x_t=xt, t=tb)
        model_mean, _, _ = gd.q_posterior(x_start=pred.pred_x_start, x_t=xt, t=tb)
        lv_p = lvp_table[t]
        if t == 0:
            term = -flat_mean(decoder_ll(x0, model_mean, 0.5 * lv_p)) / ln2
        else:
            kl = 0.5 * (-1.0 + lv_p - lv_q + torch.exp(lv_q - lv_p) + (true_mean - model_mean) ** 2 * torch.exp(-lv_p))
            term = flat_mean(kl) / ln2
            kcs.append(float(0.5 * (-1.0 + lv_p - lv_q.flatten()[0] + torch.exp(lv_q.flatten()[0] - lv_p))))
        vb.append(term)
        xs_mse.append(flat_mean((pred.pred_x_start - x0) ** 2))
        mse.append(flat_mean((pred.pred_noise - eps) ** 2))
    a = gd.alphas_cumprod[-1]
    prior = flat_mean(0.5 * (-1.0 - torch.log(1.0 - a) + (1.0 - a) + a * x0 ** 2)) / ln2
    return dict(vb=torch.stack(vb), xstart_mse=torch.stack(xs_mse), mse=torch.stack(mse), prior=prior), kcs


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, len(CLASSES), 1
    shape = (B, 3, S, S)
    img = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(IMG_SEED)).float() / 255.0
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "K": K, "T": T, "short_T": SHORT_T, "times": np.asarray(TIMES),
          "classes": np.asarray(CLASSES), "img_seed": IMG_SEED, "img": img.numpy()}
    fx.update({f"{k}_seed": v for k, v in SEEDS.items()})
    emb = torch.randn(K + 1, 4 * dim, generator=torch.Generator().manual_seed(EMB_SEED))
    fx["label_emb.weight"] = emb.numpy()
    Pw = O.unet_init(dim=dim, channels=3, seed=seed)
    w6 = _init_weight(dim, 6, INIT_W_SEED)
    fx["sc:init_conv.weight"] = w6.numpy()

    def network(double, self_condition=False, labels=False):
        net = R.Unet(dim=dim, channels=3, self_condition=self_condition)
        net.load_state_dict(dict(Pw, **({"init_conv.weight": w6} if self_condition else {})), strict=True)
        if labels:
            net.time_mlp = _TimePlusLabel(net.time_mlp, emb)
        if double:
            net.double()
            # the time embedding takes its dtype from ``time``: hand the float64 network float64 timesteps
            net.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
        return _Guided(net, torch.tensor(CLASSES), 1.0) if labels else net

    with torch.no_grad():
        for case, objective, variance, clip, netkw in CASES:
            for steps, times in ((T, TIMES), (SHORT_T, tuple(reversed(range(SHORT_T))))):
                _, nz = O.draw_loop_noise(SEEDS[case], shape, len(times))
                got = {}
                for double in (False, True):
                    gd = R.GaussianDiffusion(network(double, **netkw), img_size=S, timesteps=steps, objective=objective)
                    gd = gd.double() if double else gd
                    x0 = (img.double() if double else img) * 2 - 1
                    got[double], kcs = bpd_terms(gd, x0, times, nz, variance, clip)
                    if double and variance == "small":
                        assert all(k == 0.0 for k in kcs), (case, steps, kcs)
                    if double and variance == "large":
                        assert all(k > 0.0 for k in kcs[1:]), (case, steps, kcs)
                f32, f64 = got[False], got[True]
                kl = [i for i, t in enumerate(times) if t > 0]
                dec = [i for i, t in enumerate(times) if t == 0]
                err = float(((f32["vb"][kl].double() - f64["vb"][kl]).abs() / f64["vb"][kl].abs()).max())
                assert bool(torch.isfinite(f64["vb"][dec]).all()) and bool(torch.isfinite(f32["vb"][dec]).all()), (case, steps)
                assert err <= 1e-3, f"{case}:{steps}: the float32 KL terms miss float64 by {err:.3e}: an ill-conditioned fixture"
                for k in ("vb", "xstart_mse", "mse", "prior"):
                    assert f32[k].dtype == torch.float32 and f64[k].dtype == torch.float64
                    fx[f"{case}:{steps}:{k}"] = f32[k].numpy()
                    fx[f"{case}:{steps}:{k}64"] = f64[k].numpy()
                if steps == SHORT_T:
                    for tag, r in (("", f32), ("64", f64)):
                        total = r["vb"].sum(0) + r["prior"]
                        fx[f"{case}:{steps}:total{tag}"] = total.numpy()
                    t64 = fx[f"{case}:{steps}:total64"]
                    assert np.allclose(t64, f64["vb"].numpy().sum(0) + f64["prior"].numpy(), rtol=1e-14, atol=0)
                print(f"{case}:{steps}: KL fp32 vs fp64 {err:.3e}; decoder {f64['vb'][dec].flatten().tolist()[:2]}; prior "
                      f"{float(f64['prior'][0]):.3e}; vb[0] {float(f64['vb'][0][0]):.4e}"
                      + (f"; total {float(fx[f'{case}:{steps}:total64'][0]):.4f}" if steps == SHORT_T else ""))
    return {k: np.asarray(v) for k, v in fx.items()}


if __name__ == "__main__":
    fx = generate()
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as d:
            np.savez_compressed(os.path.join(d, "again.npz"), **fx)
            same = open(os.path.join(d, "again.npz"), "rb").read() == open(OUT, "rb").read()
        print(f"{OUT}: {'identical' if same else 'DIFFERS'}")
        sys.exit(0 if same else 1)
    np.savez_compressed(OUT, **fx)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "diffusion_inpaint.npz"))
