"""Generate tests/golden/diffusion_inpaint.npz: inpainting chains (RePaint, Lugmayr et al. 2022, Algorithm 1) around the REAL
reference's ``Unet`` and ``GaussianDiffusion.model_predictions`` on CPU.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_dynthresh.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count, ``--check`` mode, solver plan (tools/make_golden_dpmpp.py), thresholding and int8 residual packing it shares: it runs
where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_inpaint.py [--check]

The reference has no inpainting.  The loops of this file step as the loops of tools/make_golden_dynthresh.py step (the
reference's q_posterior for the ancestral chain, its ddim_sample loop body, DPM-Solver++ with the plan of
tools/make_golden_dpmpp.py) and then, written from the formulas and not imported from lgm_hip,
    known_s = M_a known + M_n eps_k                      M_a = sqrt(acp_s), M_n = sqrt(1 - acp_s); (1, 0) on the clean image
    y       = m known_s + (1 - m) x_s                    m = 1: keep the known pixel
    x       = y, or J_x y + J_n eps_j after a jump       J_x = sqrt(acp_u / acp_s), J_n = sqrt(1 - acp_u / acp_s)
along RePaint's ``get_schedule_jump`` over the sampler's levels (level n - 1 the first time, 0 the last, -1 clean): jumps[l] =
resamples - 1 for l in range(0, n - jump_length, jump_length), one level down at a time, up ``jump_length`` levels on arriving
at a level with jumps left.  A step down and the jump after it are one step; every monotone run of the walk is a DPM-Solver++
chain of its own (first-order after a jump).  The x0 handed to a self-conditioned network is the step's own clipped
prediction, not blended.  The four scalars are computed in float64 and, for the float32 chain, rounded once.

The recipe is the "small" network (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16, B = 4), T = 1000 with 10 pairs on the
reference's DDIM grid, or a timesteps=20 diffusion for the ancestral chain.  Draws: oracle.diffusion.draw_loop_noise(seed,
shape, 3 * steps) - the start image, then (noise, eps_k, eps_j) of step i at 3 i, 3 i + 1, 3 i + 2, drawn whether read or not.
The given image is uniform noise in [0, 1] ("known", seed KNOWN_SEED); one mask per sample ("mask" [B, H, W]): left half,
centre box, checkerboard, and a soft ramp with values strictly inside (0, 1).  Chains (name = the key's middle part):
    ancestral  20 levels, (jump_length, resamples) = (5, 2), pred_v and pred_noise
    ddim0 / ddim1  DDIM at eta 0 / 1, 10 levels, (3, 2), both objectives
    ode2m      2M ODE, (3, 2), pred_v              plain  2M ODE with resamples = 1, pred_v
    selfcond   2M ODE (3, 2) on the self-conditioned network of tools/make_golden_selfcond.py, pred_v
    guided     2M ODE (3, 2), thresholded at p = 0.995 and guided at scale 3 with the wrappers, embedding and classes of
               tools/make_golden_classcond.py, pred_v
Stored per chain: the final image ((x + 1) / 2, "<objective>:<chain>") in float32 and, as an int8 residual (``pack64`` of
tools/make_golden_dynthresh.py), in float64.

Asserted at generation time: every binary mask keeps between 25 % and 75 % of its sample's pixels; every result differs from
the mask-free chain (m = 0 everywhere) on the same draws by more than 1e-2 relative where m = 0; where m = 1 it equals the
given image to 1e-6.
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
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_inpaint.npz")

from tools.make_golden_classcond import CLASSES, EMB_SEED, K, SCALE, _Guided, _TimePlusLabel  # noqa: E402
from tools.make_golden_dpmpp import plan  # noqa: E402
from tools.make_golden_dynthresh import pack64, threshold  # noqa: E402
from tools.make_golden_selfcond import INIT_W_SEED, _init_weight  # noqa: E402

STEPS, T, ANCESTRAL_T, P = 10, 1000, 20, 0.995
KNOWN_SEED = 9400
# (objective, chain name, kind, (jump_length, resamples), extras)
CHAINS = [("pred_v", "ancestral", "ancestral", (5, 2), {}), ("pred_noise", "ancestral", "ancestral", (5, 2), {}),
          ("pred_v", "ddim0", "ddim", (3, 2), dict(eta=0.0)), ("pred_noise", "ddim0", "ddim", (3, 2), dict(eta=0.0)),
          ("pred_v", "ddim1", "ddim", (3, 2), dict(eta=1.0)), ("pred_noise", "ddim1", "ddim", (3, 2), dict(eta=1.0)),
          ("pred_v", "ode2m", "dpm", (3, 2), {}), ("pred_v", "plain", "dpm", (1, 1), {}),
          ("pred_v", "selfcond", "dpm", (3, 2), dict(self_condition=True)),
          ("pred_v", "guided", "dpm", (3, 2), dict(labels=True, p=P))]
SEEDS = {"ancestral": 9401, "ddim0": 9402, "ddim1": 9403, "ode2m": 9404, "plain": 9405, "selfcond": 9406, "guided": 9407}


def schedule_jump(n, jump_length, resamples):
    """RePaint's get_schedule_jump on levels n - 1 .. 0, then -1"""
    jumps = {l: resamples - 1 for l in range(0, n - jump_length, jump_length)}
    t, ts = n, []
    while t >= 1:
        t -= 1
        ts.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] -= 1
            for _ in range(jump_length):
                t += 1
                ts.append(t)
    ts.append(-1)
    return ts


def forwards(levels):
    """[(l, s, u)]: the network runs at level l, the step lands on s = l - 1 and is followed by a jump up to u (u == s: none)"""
    out, i = [], 0
    while i + 1 < len(levels):
        assert levels[i + 1] == levels[i] - 1
        j = i + 1
        while j + 1 < len(levels) and levels[j + 1] > levels[j]:
            j += 1
        out.append((levels[i], levels[i + 1], levels[j]))
        i = j
    return out


def masks(B, S):
    m = torch.zeros(B, S, S)
    m[0, :, :S // 2] = 1.0                                            # left half kept
    m[1] = 1.0
    m[1, 3:13, 3:13] = 0.0                                            # a 10 x 10 centre box to fill in
    ii, jj = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    m[2] = ((ii + jj) % 2 == 0).float()                               # checkerboard
    m[3] = (0.1 + 0.8 * jj.float() / (S - 1)) * torch.ones(S, S)      # soft: a ramp from 0.1 to 0.9
    for b in range(3):
        keep = float(m[b].mean())
        assert 0.25 <= keep <= 0.75 and set(m[b].unique().tolist()) == {0.0, 1.0}, (b, keep)
    assert 0.0 < float(m[3].min()) and float(m[3].max()) < 1.0
    return m


def inpaint_chain(gd, kind, init, nz, known, mask, jump, dtype, eta=0.0, p=None):
    """-> final image in [0, 1].  ``known`` normalised, ``mask`` [B, 1, H, W]; nz[3 i + k]: the draws of step i"""
    acp = gd.alphas_cumprod.double().tolist()
    if kind == "ancestral":
        grid = list(range(gd.num_timesteps))
    else:
        from oracle import diffusion as O
        grid = [t for t, _ in reversed(O.ddim_time_pairs(T, STEPS))]
    time = lambda l: grid[l] if l >= 0 else -1  # noqa: E731
    steps = forwards(schedule_jump(len(grid), *jump))
    rows, run = [], []
    if kind == "dpm":                                                 # every monotone run is a solver chain of its own
        for l, s, u in steps:
            run.append((time(l), time(s)))
            if u != s or s < 0:
                rows += plan(acp, run, 2, False)
                run = []
    cast = lambda v: torch.tensor(v, dtype=torch.float64).to(dtype)  # noqa: E731
    x, xs, prev = init.to(dtype), None, None
    known, mask = known.to(dtype), mask.to(dtype)
    for i, (l, s, u) in enumerate(steps):
        t, t_next = time(l), time(s)
        n0, ek, ej = (nz[3 * i + k].to(dtype) for k in range(3))
        tb = torch.full((x.shape[0],), t, dtype=torch.long)
        sc = xs if gd.self_condition else None
        if p is None:
            xs = gd.model_predictions(x, tb, sc, clip_x_start=True).pred_x_start
        else:
            xs, _ = threshold(gd.model_predictions(x, tb, sc, clip_x_start=False).pred_x_start, p)
        if kind == "ancestral":
            mean, _, logvar = gd.q_posterior(x_start=xs, x_t=x, t=tb)
            new = mean + (0.5 * logvar).exp() * n0 if t > 0 else mean
        elif kind == "ddim":
            if t_next < 0:
                new = xs
            else:
                eps = gd.predict_noise_from_start(x, tb, xs)
                alpha, alpha_next = gd.alphas_cumprod[t], gd.alphas_cumprod[t_next]
                sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
                c = (1 - alpha_next - sigma ** 2).sqrt()
                new = xs * alpha_next.sqrt() + c * eps
                if eta != 0.0:
                    new = new + sigma * n0
        else:
            kx, k0, k1, _ = (cast(v) for v in rows[i])
            new = kx * x + k0 * xs
            if float(k1) != 0.0:
                new = new + k1 * prev
            prev = xs
        a_s = acp[t_next] if s >= 0 else 1.0
        ma, mn = (math.sqrt(a_s), math.sqrt(1.0 - a_s)) if s >= 0 else (1.0, 0.0)
        known_s = cast(ma) * known + cast(mn) * ek
        x = mask * known_s + (1 - mask) * new
        if u != s:
            ratio = acp[time(u)] / a_s
            x = cast(math.sqrt(ratio)) * x + cast(math.sqrt(1.0 - ratio)) * ej
    return (x + 1) * 0.5


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, len(CLASSES), 1
    shape = (B, 3, S, S)
    known01 = torch.rand(shape, generator=torch.Generator().manual_seed(KNOWN_SEED))
    mask = masks(B, S)
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "K": K, "T": T, "steps": STEPS, "ancestral_T": ANCESTRAL_T,
          "cond_scale": np.float32(SCALE), "classes": np.asarray(CLASSES), "p": np.float64(P), "known_seed": KNOWN_SEED,
          "known": known01.numpy(), "mask": mask.numpy()}
    fx.update({f"{k}_seed": v for k, v in SEEDS.items()})
    fx.update({f"{name}_jump": np.asarray(jump) for _, name, _, jump, _ in CHAINS})
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
        return _Guided(net, torch.tensor(CLASSES), SCALE) if labels else net

    m4 = mask[:, None]
    keep, fill = (m4 == 1).expand(shape), (m4 == 0).expand(shape)
    with torch.no_grad():
        for o, name, kind, jump, extra in CHAINS:
            extra = dict(extra)
            netkw = {k: extra.pop(k) for k in ("self_condition", "labels") if k in extra}
            levels = ANCESTRAL_T if kind == "ancestral" else STEPS
            n_fwd = len(forwards(schedule_jump(levels, *jump)))
            init, nz = O.draw_loop_noise(SEEDS[name], shape, 3 * n_fwd)
            got = {}
            for double in (False, True):
                gd = R.GaussianDiffusion(network(double, **netkw), img_size=S, timesteps=levels if kind == "ancestral" else T,
                                         objective=o)
                gd = gd.double() if double else gd
                dtype = torch.float64 if double else torch.float32
                got[double] = inpaint_chain(gd, kind, init, nz, known01 * 2 - 1, m4, jump, dtype, **extra)
                if not double:
                    free = inpaint_chain(gd, kind, init, nz, known01 * 2 - 1, torch.zeros_like(m4), jump, dtype, **extra)
            img = got[False]
            d_fill = float((img - free)[fill].norm() / free[fill].norm())
            d_keep = float((img - known01)[keep].abs().max())
            print(f"{o}:{name}: {n_fwd} forwards, unknown region vs the mask-free chain {d_fill:.3e}, known region vs the given "
                  f"image {d_keep:.3e}, fp32 vs fp64 {float((img.double() - got[True]).norm() / got[True].norm()):.3e}")
            assert d_fill > 1e-2, f"{o}:{name}: the known region does not reach the generated one ({d_fill:.3e})"
            assert d_keep <= 1e-6, f"{o}:{name}: the known region is not the given image ({d_keep:.3e})"
            assert bool(torch.isfinite(img).all())
            pack64(fx, f"{o}:{name}", img.numpy(), got[True].numpy())
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
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "diffusion_selfcond.npz"))
