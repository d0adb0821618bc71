"""Generate tests/golden/diffusion_dynthresh.npz: sampling chains with dynamic thresholding of x0 (Saharia et al. 2022, 2.3)
around the REAL reference's ``Unet`` and ``GaussianDiffusion.model_predictions(..., clip_x_start=False)`` on CPU.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_dpmpp.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count, ``--check`` mode and solver plan it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_dynthresh.py [--check]

The reference has no dynamic thresholding.  The loops of this file take the reference's own unclipped x_start and threshold
it, written from the formula, not imported from lgm_hip:
    s = torch.quantile(x0.flatten(1).abs(), p, dim=1).clamp(min=1)          x0 <- clamp(x0, -s, s) / s
and then step as the reference's loops step with the clipped x_start: DPM-Solver++ with the plan of tools/make_golden_dpmpp.py,
DDIM (ddim_sample's loop body, the noise re-derived from the thresholded x0 with the reference's predict_noise_from_start) and
the ancestral chain (p_sample: the reference's q_posterior around the thresholded x0).  Each chain runs in float32 and, for
the arbiter, in float64 on the reference's modules cast to float64.

The recipe is the "small" network (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16, B = 4), T = 1000, 10 pairs on the
reference's DDIM grid, draws replayed with oracle.diffusion.draw_loop_noise.  Chains (name = the key's middle part):
    ode2m      2M ODE at p = 0.995, pred_v and pred_noise            ode2m_p95  2M ODE at p = 0.95, pred_v
    sde2m      2M SDE at 0.995, pred_v                               ddim0 / ddim1  DDIM at eta 0 / 1 at 0.995, both objectives
    ancestral  20 ancestral steps on a timesteps=20 diffusion, pred_v
    selfcond   2M ODE on the self-conditioned network of tools/make_golden_selfcond.py, pred_v
    guided     2M ODE guided at scale 3 with the wrappers, embedding and classes of tools/make_golden_classcond.py, pred_v
Stored per chain, in both precisions: the final image ((x + 1) / 2, "<objective>:<chain>"), the thresholded x0 of the first
step ("<objective>:<chain>:x0_first") and s per (step, sample) ("<objective>:<chain>:s", float64 as "...:s64").  The file may
not outgrow diffusion_dpmpp.npz, and thresholded images do not compress the way clamped ones do (nothing saturates), so a
float64 image e is stored as what the arbiter needs of it - its distance from the float32 image f of the same key: the
residual e - f as int8 in units of "<key>:r64_scale" = max|e - f| / 127 ("<key>:r64"; ``unpack64`` puts it back).  The rounding
of the residual is at most scale / 2 = max|e - f| / 254 per element, about 1 % of the distance |e - f| the arbiter compares
with (the residuals are 2e-7 ... 4e-6 here), and far below the 1e-4 the tests ask of the float32 images.

At generation time every chain must have s > 1 in at least half of its (step, sample) pairs - thresholding that never acts
checks nothing - and the p = 0.95 chain must also meet the floor s == 1 at least once.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_dynthresh.npz")

from tools.make_golden_classcond import CLASSES, EMB_SEED, K, SCALE, _Guided, _TimePlusLabel  # noqa: E402
from tools.make_golden_dpmpp import plan  # noqa: E402
from tools.make_golden_selfcond import INIT_W_SEED, _init_weight  # noqa: E402

STEPS, T, ANCESTRAL_T = 10, 1000, 20
P_DEFAULT, P_LOW = 0.995, 0.95
# (objective, chain name, kind, percentile, extras)
CHAINS = [("pred_v", "ode2m", "dpm", P_DEFAULT, {}), ("pred_noise", "ode2m", "dpm", P_DEFAULT, {}),
          ("pred_v", "ode2m_p95", "dpm", P_LOW, {}), ("pred_v", "sde2m", "dpm", P_DEFAULT, dict(stochastic=True)),
          ("pred_v", "ddim0", "ddim", P_DEFAULT, dict(eta=0.0)), ("pred_noise", "ddim0", "ddim", P_DEFAULT, dict(eta=0.0)),
          ("pred_v", "ddim1", "ddim", P_DEFAULT, dict(eta=1.0)), ("pred_noise", "ddim1", "ddim", P_DEFAULT, dict(eta=1.0)),
          ("pred_v", "ancestral", "ancestral", P_DEFAULT, {}),
          ("pred_v", "selfcond", "dpm", P_DEFAULT, dict(self_condition=True)),
          ("pred_v", "guided", "dpm", P_DEFAULT, dict(labels=True))]
SEEDS = {"ode2m": 9301, "ode2m_p95": 9302, "sde2m": 9303, "ddim0": 9304, "ddim1": 9305, "ancestral": 9306, "selfcond": 9307,
         "guided": 9308}


def pack64(fx, key, f, e):
    """float32 result f under ``key``, float64 result e as an int8 residual (see the docstring)"""
    f, e = np.asarray(f, dtype=np.float32), np.asarray(e, dtype=np.float64)
    d = e - f.astype(np.float64)
    scale = max(float(np.abs(d).max()), 1e-300) / 127.0
    fx[key], fx[key + ":r64"], fx[key + ":r64_scale"] = f.copy(), np.rint(d / scale).astype(np.int8), np.float64(scale)


def unpack64(fx, key):
    return fx[key].astype(np.float64) + fx[key + ":r64"].astype(np.float64) * float(fx[key + ":r64_scale"])


def threshold(x0, p):
    """-> (thresholded x0, s [B]): the formula of the docstring, in x0's precision"""
    s = torch.quantile(x0.flatten(1).abs(), p, dim=1).clamp(min=1)
    sv = s.view(-1, 1, 1, 1)
    return torch.maximum(torch.minimum(x0, sv), -sv) / sv, s


def _x0(gd, x, t, xs, p):
    """the reference's unclipped x_start at the shared timestep t, thresholded"""
    tb = torch.full((x.shape[0],), t, dtype=torch.long)
    raw = gd.model_predictions(x, tb, xs if gd.self_condition else None, clip_x_start=False).pred_x_start
    return threshold(raw, p) + (tb,)


def dpm_chain(gd, init, nz, p, dtype, stochastic=False):
    """DPM-Solver++(2M) as tools/make_golden_dpmpp.py steps it -> (image in [0, 1], first x0, s [steps, B])"""
    from oracle import diffusion as O
    pairs = O.ddim_time_pairs(T, STEPS)
    rows = plan(gd.alphas_cumprod.double().tolist(), pairs, 2, stochastic)
    x, prev, first, xs, ss = init.to(dtype), None, None, None, []
    for i, ((t, _), row) in enumerate(zip(pairs, rows)):
        kx, k0, k1, kn = (torch.tensor(v, dtype=torch.float64).to(dtype) for v in row)
        xs, s, _ = _x0(gd, x, t, xs, p)
        ss.append(s)
        first = xs.clone() if first is None else first
        new = kx * x + k0 * xs
        if float(k1) != 0.0:
            new = new + k1 * prev
        if float(kn) != 0.0:
            new = new + kn * nz[i].to(dtype)
        x, prev = new, xs
    return (x + 1) * 0.5, first, torch.stack(ss)


def ddim_chain(gd, init, nz, p, dtype, eta):
    """the reference's ddim_sample loop body around the thresholded x0 and the noise re-derived from it"""
    from oracle import diffusion as O
    x, first, xs, ss = init.to(dtype), None, None, []
    for i, (t, t_next) in enumerate(O.ddim_time_pairs(T, STEPS)):
        xs, s, tb = _x0(gd, x, t, xs, p)
        ss.append(s)
        first = xs.clone() if first is None else first
        if t_next < 0:
            x = xs
            continue
        eps = gd.predict_noise_from_start(x, tb, xs)
        alpha, alpha_next = gd.alphas_cumprod[t], gd.alphas_cumprod[t_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        x = xs * alpha_next.sqrt() + c * eps
        if eta != 0.0:
            x = x + sigma * nz[i].to(dtype)
    return (x + 1) * 0.5, first, torch.stack(ss)


def ancestral_chain(gd, init, nz, p, dtype):
    """the reference's p_sample around the thresholded x0: q_posterior's mean plus sigma * noise for t > 0"""
    x, first, xs, ss = init.to(dtype), None, None, []
    for i, t in enumerate(reversed(range(gd.num_timesteps))):
        xs, s, tb = _x0(gd, x, t, xs, p)
        ss.append(s)
        first = xs.clone() if first is None else first
        mean, _, logvar = gd.q_posterior(x_start=xs, x_t=x, t=tb)
        x = mean + (0.5 * logvar).exp() * nz[i].to(dtype) if t > 0 else mean
    return (x + 1) * 0.5, first, torch.stack(ss)


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, len(CLASSES), 1
    shape = (B, 3, S, S)
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "K": K, "T": T, "steps": STEPS, "ancestral_T": ANCESTRAL_T,
          "cond_scale": np.float32(SCALE), "classes": np.asarray(CLASSES), "p": np.float64(P_DEFAULT),
          "p_low": np.float64(P_LOW)}
    fx.update({f"{k}_seed": v for k, v in SEEDS.items()})
    emb = torch.randn(K + 1, 4 * dim, generator=torch.Generator().manual_seed(EMB_SEED))
    fx["label_emb.weight"] = emb.numpy()
    P = O.unet_init(dim=dim, channels=3, seed=seed)
    w6 = _init_weight(dim, 6, INIT_W_SEED)
    fx["sc:init_conv.weight"] = w6.numpy()

    def network(double, self_condition=False, labels=False):
        net = R.Unet(dim=dim, channels=3, self_condition=self_condition)
        net.load_state_dict(dict(P, **({"init_conv.weight": w6} if self_condition else {})), strict=True)
        if labels:
            net.time_mlp = _TimePlusLabel(net.time_mlp, emb)
        if double:
            net.double()
            # the time embedding takes its dtype from ``time``: hand the float64 network float64 timesteps
            net.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
        return _Guided(net, torch.tensor(CLASSES), SCALE) if labels else net

    with torch.no_grad():
        for o, name, kind, p, extra in CHAINS:
            extra = dict(extra)
            netkw = {k: extra.pop(k) for k in ("self_condition", "labels") if k in extra}
            steps = ANCESTRAL_T if kind == "ancestral" else STEPS
            init, nz = O.draw_loop_noise(SEEDS[name], shape, steps - 1)
            got = {}
            for double in (False, True):
                gd = R.GaussianDiffusion(network(double, **netkw), img_size=S, timesteps=steps if kind == "ancestral" else T,
                                         objective=o)
                gd = gd.double() if double else gd
                run = {"dpm": dpm_chain, "ddim": ddim_chain, "ancestral": ancestral_chain}[kind]
                img, first, s = run(gd, init, nz, p, torch.float64 if double else torch.float32, **extra)
                suffix = "64" if double else ""
                got[double] = (img.numpy(), first.numpy())
                fx[f"{o}:{name}:s{suffix}"] = s.numpy().copy()
                active = float((s > 1).double().mean())
                print(f"{o}:{name}{suffix}: s > 1 in {active:.2f} of the (step, sample) pairs, s of sample 0: "
                      + " ".join(f"{float(v):.3g}" for v in s[:, 0]))
                assert active >= 0.5, f"{o}:{name}: the threshold acts in {active:.2f} of the (step, sample) pairs only"
                if name == "ode2m_p95":
                    assert bool((s == 1).any()), f"{o}:{name}: the floor s == 1 never occurs"
            pack64(fx, f"{o}:{name}", got[False][0], got[True][0])
            pack64(fx, f"{o}:{name}:x0_first", got[False][1], got[True][1])
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
