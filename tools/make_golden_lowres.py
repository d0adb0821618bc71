"""Generate tests/golden/diffusion_lowres.npz: the REAL reference's ``Unet`` / ``GaussianDiffusion`` on CPU as a
low-resolution conditioned super-resolution stage, for ``objective="pred_v"`` and ``"pred_noise"``.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_classcond.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_lowres.py [--check]

The reference has no low-resolution conditioning, but its self-conditioned network reads ``cat((x_self_cond, x), dim=1)``:
``Unet(self_condition=True)`` with ``x_self_cond :=`` the conditioning image IS the conditioned network's input layout.
``_TimePlusAug`` takes the place of ``Unet.time_mlp`` and returns ``time_mlp(t) + lowres_mlp(s)`` (+ one label-embedding row per
sample in the guided case), ``lowres_mlp`` a second ``nn.Sequential(SinusoidalPosEmb, Linear, GELU, Linear)`` of the
reference's own modules.  The conditioning image is torch's own arithmetic: ``avg_pool2d`` by r, ``* 2 - 1``, ``interpolate``
(bilinear, align_corners=False) by r, ``sqrt_ac[s] u + sqrt_1mac[s] eps``.  The loss is the textbook formula around the
network - q_sample, the objective's target, mean_b(loss_weight[t_b] mse_b) with the reference's own tables - because the
reference's ``p_losses`` would flip the self-conditioning coin; the chains are the reference's loop bodies
(``model_predictions`` / ``p_mean_variance`` with the conditioning image as ``x_self_cond``) on replayed draws.

Recipe: oracle.unet_init(dim=16, channels=3, seed=1) with a seeded [16, 6, 7, 7] ``init_conv.weight`` and a seeded
``lowres_time_mlp``, 16 x 16, r = 4, B = 4, t = (37, 912, 0, 999), s = (0, 200, 999, 50), data seed 101.  Stored per
objective: the UNet output; loss and gradients (``lowres_time_mlp.*`` and ``init_conv.weight`` whole, the others as GNAMES:
whole up to 8192 elements, else norm + strided sample); a 20-pair DDIM chain (timesteps=1000) and a 50-step ancestral chain
(timesteps=50) conditioned on the low-resolution batch at level s, each with a float64 evaluation of the same modules for the
arbiter.  One guided class-conditional case (pred_v, K = 5, classes (3, 0, 3, 5), cond_scale 3): output and unclipped x_start.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_lowres.npz")

from tools.make_golden_objectives import GNAMES, SAMPLE, WHOLE  # noqa: E402
from tools.make_golden_selfcond import INIT_W_SEED, _init_weight  # noqa: E402

OBJECTIVES = ("pred_v", "pred_noise")
R_FACTOR, TIMES, LEVELS = 4, (37, 912, 0, 999), (0, 200, 999, 50)
MLP_SEED, AUG_SEED, EMB_SEED = 811, 812, 813
K, CLASSES, SCALE = 5, (3, 0, 3, 5), 3.0
DDIM_SEED, ANCESTRAL_SEED, DDIM_STEPS, ANCESTRAL_T = 9201, 9202, 20, 50


class _TimePlusAug(nn.Module):
    """in place of ``Unet.time_mlp``: the time embedding plus the embedding of the augmentation level (plus a label row)"""

    def __init__(self, time_mlp, lowres_mlp, label=None):
        super().__init__()
        self.time_mlp, self.lowres_mlp = time_mlp, lowres_mlp
        if label is not None:
            self.weight = nn.Parameter(label.clone())
        self.s = self.classes = None

    def forward(self, t):
        e = self.time_mlp(t) + self.lowres_mlp(self.s.to(t.dtype))
        return e if self.classes is None else e + self.weight[self.classes]


def _pname(n):
    """parameter name of the wrapped network -> name in a Unet(lowres_cond=True)"""
    return n.replace("time_mlp.time_mlp.", "time_mlp.").replace("time_mlp.lowres_mlp.", "lowres_time_mlp.")


def cond_image(img, s, eps, sa, sb, r=R_FACTOR, dtype=torch.float32):
    """the conditioning image of a stage from the data-range batch, in torch's own arithmetic"""
    low = F.avg_pool2d(img.to(dtype), r)
    u = F.interpolate(low * 2 - 1, scale_factor=r, mode="bilinear", align_corners=False)
    return sa.to(dtype)[s].view(-1, 1, 1, 1) * u + sb.to(dtype)[s].view(-1, 1, 1, 1) * eps.to(dtype)


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, len(TIMES), 1
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "r": R_FACTOR, "K": K, "data_seed": 100 + seed, "aug_seed": AUG_SEED,
          "cond_scale": np.float32(SCALE), "ddim_loop_seed": DDIM_SEED, "p_sample_loop_seed": ANCESTRAL_SEED,
          "ddim_steps": DDIM_STEPS, "ancestral_T": ANCESTRAL_T, "grad_sample": SAMPLE}
    t, s, classes = torch.tensor(TIMES), torch.tensor(LEVELS), torch.tensor(CLASSES)
    fx["t"], fx["s"], fx["classes"] = t.numpy(), s.numpy(), classes.numpy()
    P = O.unet_init(dim=dim, channels=3, seed=seed)
    P["init_conv.weight"] = _init_weight(dim, 6, INIT_W_SEED)
    fx["init_conv.weight"] = P["init_conv.weight"].numpy()
    torch.manual_seed(MLP_SEED)
    mlp0 = nn.Sequential(R.SinusoidalPosEmb(dim, theta=10000), nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, 4 * dim))
    for n, p in mlp0.state_dict().items():
        fx[f"lowres_time_mlp.{n}"] = p.numpy().copy()
    emb = torch.randn(K + 1, 4 * dim, generator=torch.Generator().manual_seed(EMB_SEED))
    fx["label_emb.weight"] = emb.numpy()

    def network(double=False, label=False):
        net = R.Unet(dim=dim, channels=3, self_condition=True)
        net.load_state_dict(P, strict=True)
        mlp = nn.Sequential(R.SinusoidalPosEmb(dim, theta=10000), nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, 4 * dim))
        mlp.load_state_dict(mlp0.state_dict())
        net.time_mlp = _TimePlusAug(net.time_mlp, mlp, emb if label else None)
        if double:
            net.double()
            net.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
        return net

    unet, unet64 = network(), network(double=True)
    ref_names = list(R.Unet(dim=dim, channels=3, self_condition=True).state_dict().keys())
    fx["sd_names"] = np.asarray(ref_names + [f"lowres_time_mlp.{n}" for n in mlp0.state_dict()])
    g = torch.Generator().manual_seed(100 + seed)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)
    eps = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(AUG_SEED))
    x0 = img * 2 - 1
    shape = (B, 3, S, S)
    fx["low"] = F.avg_pool2d(img, R_FACTOR).numpy()

    def ancestral(gd, net, cond, init, nz):
        x = init.to(cond.dtype)
        for i, ti in enumerate(reversed(range(gd.num_timesteps))):
            tb = torch.full((B,), ti, dtype=torch.long)
            mean, _, logvar, _ = gd.p_mean_variance(x, tb, cond, clip_denoised=True)
            x = mean + (0.5 * logvar).exp() * nz[i].to(cond.dtype) if ti > 0 else mean
        return (x + 1) * 0.5

    def ddim(gd, net, cond, init, nz):
        x = init.to(cond.dtype)
        for i, (ti, tn) in enumerate(O.ddim_time_pairs(gd.num_timesteps, DDIM_STEPS)):
            tb = torch.full((B,), ti, dtype=torch.long)
            pn, xs = gd.model_predictions(x, tb, cond, clip_x_start=True, rederive_pred_noise=True)
            if tn < 0:
                x = xs
                continue
            a, an = gd.alphas_cumprod[ti], gd.alphas_cumprod[tn]
            x = xs * an.sqrt() + (1 - an).sqrt() * pn
        return (x + 1) * 0.5

    for o in OBJECTIVES:
        mk = lambda net, **kw: R.GaussianDiffusion(net, img_size=S, objective=o, **kw)  # noqa: E731
        gd = mk(unet, timesteps=1000)
        cond = cond_image(img, s, eps, gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod)
        fx[f"{o}:cond"] = cond.numpy()
        x_t = gd.q_sample(x0, t, noise)
        fx[f"{o}:x_t"] = x_t.numpy()
        unet.time_mlp.s = unet64.time_mlp.s = s
        with torch.no_grad():
            fx[f"{o}:unet_out"] = unet(x_t, t, cond).numpy()
        for p in unet.parameters():
            p.grad = None
        out = unet(x_t, t, cond)
        target = {"pred_noise": noise, "pred_v": gd.predict_v(x0, t, noise)}[o]
        loss = (((out - target) ** 2).reshape(B, -1).mean(1) * gd.loss_weight[t]).mean()
        loss.backward()
        fx[f"{o}:loss"] = loss.detach().numpy()
        named = {_pname(n): p for n, p in unet.named_parameters()}
        whole = ["init_conv.weight"] + [n for n in named if n.startswith("lowres_time_mlp.")]
        for n in dict.fromkeys(whole + GNAMES):
            flat = named[n].grad.reshape(-1)
            if flat.numel() <= WHOLE or n in whole:
                fx[f"{o}:grad:{n}"] = named[n].grad.numpy().copy()
            else:
                fx[f"{o}:gradnorm:{n}"] = np.float64(flat.double().norm().item())
                fx[f"{o}:gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[f"{o}:gradnorm_all"] = np.float64(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in unet.parameters())).item())
        with torch.no_grad():
            gd_d, gd_d64 = mk(unet, timesteps=1000), mk(unet64, timesteps=1000).double()
            cond64 = cond_image(img, s, eps, gd_d64.sqrt_alphas_cumprod, gd_d64.sqrt_one_minus_alphas_cumprod, dtype=torch.float64)
            init, nz = O.draw_loop_noise(DDIM_SEED, shape, DDIM_STEPS - 1)
            fx[f"{o}:ddim_loop"] = ddim(gd_d, unet, cond, init, nz).numpy()
            fx[f"{o}:ddim_loop64"] = ddim(gd_d64, unet64, cond64, init, nz).numpy()
            gd_a, gd_a64 = mk(unet, timesteps=ANCESTRAL_T), mk(unet64, timesteps=ANCESTRAL_T).double()
            sa_ = torch.clamp(s, max=ANCESTRAL_T - 1)             # the levels inside the 50-step schedule
            fx["s_ancestral"] = sa_.numpy()
            unet.time_mlp.s = unet64.time_mlp.s = sa_
            cond_a = cond_image(img, sa_, eps, gd_a.sqrt_alphas_cumprod, gd_a.sqrt_one_minus_alphas_cumprod)
            cond_a64 = cond_image(img, sa_, eps, gd_a64.sqrt_alphas_cumprod, gd_a64.sqrt_one_minus_alphas_cumprod,
                                  dtype=torch.float64)
            init, nz = O.draw_loop_noise(ANCESTRAL_SEED, shape, ANCESTRAL_T - 1)
            fx[f"{o}:p_sample_loop"] = ancestral(gd_a, unet, cond_a, init, nz).numpy()
            fx[f"{o}:p_sample_loop64"] = ancestral(gd_a64, unet64, cond_a64, init, nz).numpy()
        print(f"{o}: loss {float(loss.detach()):.6f}")

    # guided class-conditional stage (pred_v): out_null + 3 (out_cond - out_null), then the unclipped x_start
    netc, netc64 = network(label=True), network(double=True, label=True)
    gd = R.GaussianDiffusion(netc, img_size=S, objective="pred_v", timesteps=1000)
    gd64 = R.GaussianDiffusion(netc64, img_size=S, objective="pred_v", timesteps=1000).double()
    cond = torch.as_tensor(fx["pred_v:cond"])
    cond64 = cond_image(img, s, eps, gd64.sqrt_alphas_cumprod, gd64.sqrt_one_minus_alphas_cumprod, dtype=torch.float64)
    x_t = torch.as_tensor(fx["pred_v:x_t"])
    null = torch.full_like(classes, K)

    def guided(net, g_, x, c):
        net.time_mlp.s = s
        net.time_mlp.classes = classes
        oc = net(x, t, c)
        net.time_mlp.classes = null
        on = net(x, t, c)
        v = on + SCALE * (oc - on)
        return oc, v, g_.predict_start_from_v(x, t, v)
    with torch.no_grad():
        oc, v, xs = guided(netc, gd, x_t, cond)
        fx["guided:unet_out:cond"], fx["guided:unet_out:mix"], fx["guided:x_start"] = oc.numpy(), v.numpy(), xs.numpy()
        fx["guided:x_start64"] = guided(netc64, gd64, x_t.double(), cond64)[2].numpy()
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
