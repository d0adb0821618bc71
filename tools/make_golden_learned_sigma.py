"""Generate tests/golden/diffusion_learned_sigma.npz: the hybrid loss (Nichol & Dhariwal 2021, L_hybrid), one ancestral step
with the learned variance and the variational bound with it, around the REAL reference's ``Unet(learned_variance=True)`` on CPU.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_bpd.py, whose stubs (oracle.make_golden.install_stubs), pinned thread count,
``decoder_ll`` and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_learned_sigma.py [--check]

The reference builds the network (``out_dim = 2 * channels``) but its ``GaussianDiffusion`` refuses it, so everything around the
network is written here from the formulas, in their textbook form and not imported from lgm_hip.  With the network output split
into (pred, v), f = (v + 1) / 2 and lv = f log beta_t + (1 - f) log beta~_t (log beta~_1 at t = 0):
    x_t = q_sample(x0, t, eps);  x0_pred = sqrt_ac x_t - sqrt_1mac pred  (pred_v);  mean = P1 x0_pred + P2 x_t
    t >= 1:  term = 0.5 (-1 + lv - lv_q + exp(lv_q - lv) + (true_mean - mean)^2 exp(-lv))
    t == 0:  term = -discretised Gaussian log-likelihood of x0 under (mean, 0.5 lv)
    training   L = mean_b(lw[t_b] mse_b) + VB_WEIGHT mean_b(vb_b),  vb_b = mean(term) / ln 2, the mean DETACHED and x0_pred unclipped
    p_sample   x_{t-1} = mean + exp(0.5 lv) noise (t > 0), x0_pred clipped to [-1, 1]
    bound      the terms with x0_pred clipped, beside them mean (x0_pred - x0)^2 and mean (eps_pred - eps)^2, and the prior

The recipe is the "small" network (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16) with a final_conv of 6 channels drawn
from HEAD_SEED (its weight HEAD_GAIN times the fan-in bound), a cosine schedule of T = 8, pred_v, B = 4 with t = (0, 1, 4, 7), 8-bit-quantised uniform images.  Every quantity
twice: float32 (key) and float64 with torch autograd (key + "64").  Stored: loss, mse_b (weighted), vb_b; the gradient with
respect to the network output, all 6 channels ("gout"); every parameter gradient in float64 ("grad:<name>", or
"gradnorm:<name>" and "gradsample:<name>" above WHOLE elements) with the float32 evaluation's distance from it ("dref:<name>"); p_sample at t = 0, 1, 7 from
"ps:x" with the draw "ps:noise"; the reference network's state-dict names and shapes ("sd_names", "sd_shapes"); the bound over all 8 timesteps with the draws "vlb:noise"; and "gvar_dist", the relative L2
distance of the float32 variance-lane gradient from the float64 one - the yardstick of the device's.

Asserted at generation time, in float64: the variance-lane gradient is non-zero for every sample, t = 0 included; the t = 0
sample has an element in an end bin and an element whose probability is floored.
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
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_learned_sigma.npz")

from tools.make_golden_bpd import approx_cdf, decoder_ll  # noqa: E402

T, TIMES, PS_TIMES = 8, (0, 1, 4, 7), (0, 1, 7)
DIM, S, B, SEED = 16, 16, 4, 1
IMG_SEED, HEAD_SEED, NOISE_SEED, PS_SEED, VLB_SEED = 9700, 9701, 9702, 9703, 9704
VB_WEIGHT = 0.001
WHOLE, SAMPLE = 512, 256
HEAD_GAIN = 4        # the head's weights above their fan-in bound: residuals beyond 6 sigma at t = 0 and f outside [0, 1]
LN2 = math.log(2.0)


def cosine_tables(dtype):
    """the schedule's tables from the formulas, float64, cast once (the reference's order of operations)"""
    t = torch.linspace(0, T, T + 1, dtype=torch.float64) / T
    ac = torch.cos((t + 0.008) / 1.008 * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    betas = torch.clip(1 - ac[1:] / ac[:-1], 0, 0.999)
    acp = torch.cumprod(1 - betas, 0)
    prev = torch.cat([torch.ones(1, dtype=torch.float64), acp[:-1]])
    post = betas * (1 - prev) / (1 - acp)
    lvq = torch.log(post.clamp(min=1e-20))
    tab = dict(sa=acp.sqrt(), s1=(1 - acp).sqrt(), R=(1 / acp).sqrt(), Rm1=(1 / acp - 1).sqrt(), lvq=lvq,
               lt=torch.cat([lvq[1:2], lvq[1:]]), lb=torch.log(betas), P1=betas * prev.sqrt() / (1 - acp),
               P2=(1 - prev) * (1 - betas).sqrt() / (1 - acp), lw=acp, acp=acp)     # pred_v: snr / (snr + 1) = acp
    return {k: v.to(dtype) for k, v in tab.items()}


def ex(tab, name, t):
    return tab[name][t][:, None, None, None]


def flat_mean(x):
    return x.flatten(1).mean(1)


def terms(tab, t, x0, xt, pred, v, clip):
    """-> (term per element in nats, x0_pred, mean) with the mean detached"""
    x0p = (ex(tab, "sa", t) * xt - ex(tab, "s1", t) * pred).detach()
    if clip:
        x0p = x0p.clamp(-1.0, 1.0)
    mean = ex(tab, "P1", t) * x0p + ex(tab, "P2", t) * xt
    true_mean = ex(tab, "P1", t) * x0 + ex(tab, "P2", t) * xt
    f = (v + 1) / 2
    lv = f * ex(tab, "lb", t) + (1 - f) * ex(tab, "lt", t)
    lvq = ex(tab, "lvq", t)
    kl = 0.5 * (-1.0 + lv - lvq + torch.exp(lvq - lv) + (true_mean - mean) ** 2 * torch.exp(-lv))
    dec = -decoder_ll(x0, mean, 0.5 * lv)
    return torch.where((t == 0)[:, None, None, None], dec, kl), x0p, mean, lv


def hybrid(net, tab, x0, t, eps):
    xt = ex(tab, "sa", t) * x0 + ex(tab, "s1", t) * eps
    out = net(xt, t)
    out.retain_grad()
    pred, v = out.chunk(2, dim=1)
    target = ex(tab, "sa", t) * eps - ex(tab, "s1", t) * x0
    mse_b = flat_mean((pred - target) ** 2) * tab["lw"][t]
    term, x0p, mean, lv = terms(tab, t, x0, xt, pred, v, clip=False)
    vb_b = flat_mean(term) / LN2
    loss = mse_b.mean() + VB_WEIGHT * vb_b.mean()
    return loss, mse_b, vb_b, out, (x0p, mean, lv)


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    shape = (B, 3, S, S)
    g = lambda seed: torch.Generator().manual_seed(seed)  # noqa: E731
    img = torch.randint(0, 256, shape, generator=g(IMG_SEED)).float() / 255.0
    Pw = O.unet_init(dim=DIM, channels=3, seed=SEED)
    hg = g(HEAD_SEED)
    bound = 1.0 / math.sqrt(DIM)
    head_w = (torch.rand(6, DIM, 1, 1, generator=hg) * 2 - 1) * bound * HEAD_GAIN
    head_b = (torch.rand(6, generator=hg) * 2 - 1) * bound
    eps = torch.randn(shape, generator=g(NOISE_SEED))
    ps_x = torch.randn(shape, generator=g(PS_SEED))
    ps_noise = torch.randn(shape, generator=g(PS_SEED + 100))
    vlb_noise = torch.randn((T,) + shape, generator=g(VLB_SEED))
    t = torch.tensor(TIMES)
    fx = {"T": T, "times": np.asarray(TIMES), "ps_times": np.asarray(PS_TIMES), "dim": DIM, "S": S, "B": B, "seed": SEED,
          "vb_weight": VB_WEIGHT, "img": img.numpy(), "noise": eps.numpy(), "final_conv.weight": head_w.numpy(),
          "final_conv.bias": head_b.numpy(), "ps:x": ps_x.numpy(), "ps:noise": ps_noise.numpy(), "vlb:noise": vlb_noise.numpy()}

    def network(double):
        net = R.Unet(dim=DIM, channels=3, learned_variance=True)
        net.load_state_dict(dict(Pw, **{"final_conv.weight": head_w, "final_conv.bias": head_b}), strict=True)
        if double:
            net.double()
            net.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
        return net

    sd = network(False).state_dict()                         # the reference's names and shapes, in its order
    fx["sd_names"] = np.asarray(list(sd.keys()))
    fx["sd_shapes"] = np.asarray([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()])
    got, grads = {}, {}
    for double in (False, True):
        tag = "64" if double else ""
        dtype = torch.float64 if double else torch.float32
        tab, net = cosine_tables(dtype), network(double)
        x0 = img.to(dtype) * 2 - 1
        loss, mse_b, vb_b, out, (x0p, mean, lv) = hybrid(net, tab, x0, t, eps.to(dtype))
        loss.backward()
        got[double] = out.grad.detach().clone()
        fx["loss" + tag], fx["mse_b" + tag], fx["vb_b" + tag] = (a.detach().numpy() for a in (loss, mse_b, vb_b))
        fx["unet_out" + tag], fx["gout" + tag] = out.detach().numpy(), out.grad.numpy()
        grads[double] = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        if double:
            gv = out.grad[:, 3:]
            assert all(float(gv[b].abs().max()) > 0.0 for b in range(B)), "a sample without a variance-lane gradient"
            x00, z = x0[0], (x0[0] - mean[0]) * torch.exp(-0.5 * lv[0].detach())
            end = (x00 < -0.999) | (x00 > 0.999)
            inv = torch.exp(-0.5 * lv[0].detach())
            delta = approx_cdf(inv * (x00 - mean[0] + 1 / 255)) - approx_cdf(inv * (x00 - mean[0] - 1 / 255))
            floored = (~end) & (delta < 1e-12)
            print(f"t = 0 sample: {int(end.sum())} end-bin elements, {int(floored.sum())} floored, max |z| {float(z.abs().max()):.2f}")
            assert int(end.sum()) > 0 and int(floored.sum()) > 0, "choose images / seeds with an end bin and a floored bin at t = 0"
            assert float(gv[0].abs().max()) > 0.0
        with torch.no_grad():
            for ti in PS_TIMES:
                tb = torch.full((B,), ti, dtype=torch.long)
                xt = ps_x.to(dtype)
                pred, v = net(xt, tb).chunk(2, dim=1)
                _, x0p, mean, lv = terms(tab, tb, xt, xt, pred, v, clip=True)
                nxt = mean + torch.exp(0.5 * lv) * ps_noise.to(dtype) if ti > 0 else mean
                fx[f"ps:{ti}:out{tag}"], fx[f"ps:{ti}:x0{tag}"] = nxt.numpy(), x0p.numpy()
            vb, xs, ms = [], [], []
            for i, ti in enumerate(reversed(range(T))):
                tb = torch.full((B,), ti, dtype=torch.long)
                e = vlb_noise[i].to(dtype)
                xt = ex(tab, "sa", tb) * x0 + ex(tab, "s1", tb) * e
                pred, v = net(xt, tb).chunk(2, dim=1)
                term, x0p, _, _ = terms(tab, tb, x0, xt, pred, v, clip=True)
                e_pred = (ex(tab, "R", tb) * xt - x0p) / ex(tab, "Rm1", tb)
                vb.append(flat_mean(term) / LN2)
                xs.append(flat_mean((x0p - x0) ** 2))
                ms.append(flat_mean((e_pred - e) ** 2))
            a = tab["acp"][-1]
            prior = flat_mean(0.5 * (-1.0 - torch.log(1.0 - a) + (1.0 - a) + a * x0 ** 2)) / LN2
            vb = torch.stack(vb)
            for k, val in (("vb", vb), ("xstart_mse", torch.stack(xs)), ("mse", torch.stack(ms)), ("prior", prior),
                           ("total", vb.sum(0) + prior)):
                fx[f"vlb:{k}{tag}"] = val.numpy()
    # every parameter gradient in float64: whole up to WHOLE elements, else its norm and SAMPLE strided elements; beside each
    # the relative L2 distance of the float32 evaluation from it ("dref:<name>", over what is stored)
    for n, g64 in grads[True].items():
        f64, f32 = g64.reshape(-1), grads[False][n].reshape(-1).double()
        if f64.numel() > WHOLE:
            fx["gradnorm:" + n] = np.float64(f64.norm().item())
            step = f64.numel() // SAMPLE
            f64, f32 = f64[::step][:SAMPLE], f32[::step][:SAMPLE]
            fx["gradsample:" + n] = f64.numpy().copy()
        else:
            fx["grad:" + n] = g64.numpy().copy()
        fx["dref:" + n] = float((f32 - f64).norm() / f64.norm().clamp_min(1e-300))
    fx["gradnorm_all"] = np.float64(torch.sqrt(sum(v.pow(2).sum() for v in grads[True].values())).item())
    g32, g64 = got[False][:, 3:].double(), got[True][:, 3:]
    fx["gvar_dist"] = float((g32 - g64).norm() / g64.norm())
    m32, m64 = got[False][:, :3].double(), got[True][:, :3]
    fx["gmean_dist"] = float((m32 - m64).norm() / m64.norm())
    print(f"loss {float(fx['loss64']):.6f}  vb_b {fx['vb_b64'].tolist()}  variance-lane gradient float32 vs float64 "
          f"{fx['gvar_dist']:.3e}, prediction lanes {fx['gmean_dist']:.3e}; total bpd {fx['vlb:total64'].tolist()}")
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
    assert os.path.getsize(OUT) <= 1 << 20
