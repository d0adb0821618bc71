"""Generate tests/golden/diffusion_selfcond.npz by running the REAL reference's ``Unet(self_condition=True)`` and
``GaussianDiffusion`` on CPU, for ``objective="pred_v"`` and ``"pred_noise"``.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_objectives.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_selfcond.py [--check]

The recipe is the "small" case (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16, B = 2, t = (37, 912), data seed 101)
with ``init_conv.weight`` replaced by a seeded [16, 6, 7, 7] draw, stored in the file together with the supplied
``x_self_cond``.  The reference's coin (``random() < 0.5``, ddpm.py:902) is forced by rebinding the name ``random`` in the
reference's module to a constant function.  Stored per objective: the UNet output with the supplied x_self_cond and with
None; p_losses' loss and the gradients of GNAMES for coin off and coin on (large gradients as norm + strided sample,
init_conv.weight's whole); model_predictions with the supplied x_self_cond, clip off and on; the 200-step ancestral chain and
the 50-pair DDIM chain (eta = 0 and eta = 0.7) with the global CPU generator seeded the way tools/make_golden_objectives.py
seeds it (the tests replay the draws with oracle.diffusion.draw_loop_noise), and for every chain and for the unclipped
x_start a float64 evaluation for the arbiter: the reference's own modules cast to float64 (the float32 schedule tables,
exactly representable) on the same draws.  A one-channel network (input pitch 4, x slice at lane 1): output and loss, coin on.
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
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_selfcond.npz")

from tools.make_golden_objectives import GNAMES, SAMPLE, WHOLE  # noqa: E402

OBJECTIVES = ("pred_v", "pred_noise")
INIT_W_SEED, SC_SEED, C1_SEED = 611, 612, 613
DDIM_SEED, ANCESTRAL_SEED, DDIM_ETA_SEED, ETA = 9001, 9002, 9003, 0.7
DDIM_STEPS, ANCESTRAL_T = 50, 200


def _init_weight(dim, cin, seed):
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / (cin * 49) ** 0.5
    return (torch.rand(dim, cin, 7, 7, generator=g) * 2 - 1) * bound


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, 2, 1
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "data_seed": 100 + seed, "ddim_loop_seed": DDIM_SEED,
          "p_sample_loop_seed": ANCESTRAL_SEED, "ddim_eta_loop_seed": DDIM_ETA_SEED, "eta": np.float32(ETA),
          "ddim_steps": DDIM_STEPS, "ancestral_T": ANCESTRAL_T, "grad_sample": SAMPLE, "c1_seed": 2}
    P = O.unet_init(dim=dim, channels=3, seed=seed)
    P["init_conv.weight"] = _init_weight(dim, 6, INIT_W_SEED)
    fx["init_conv.weight"] = P["init_conv.weight"].numpy()
    unet = R.Unet(dim=dim, channels=3, self_condition=True)
    unet.load_state_dict(P, strict=True)
    sd = unet.state_dict()
    fx["sd_names"] = np.asarray(list(sd.keys()))
    fx["sd_shapes"] = np.asarray([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    unet64 = R.Unet(dim=dim, channels=3, self_condition=True)
    unet64.load_state_dict(P, strict=True)
    unet64.double()
    # the time embedding takes its dtype from ``time``: hand the float64 network float64 timesteps (the tables still index by t)
    unet64.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
    g = torch.Generator().manual_seed(100 + seed)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)
    t = torch.tensor([37, 912])
    fx["t"] = t.numpy()
    x0 = img * 2 - 1
    sc = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(SC_SEED)) * 2 - 1
    fx["x_self_cond"] = sc.numpy()
    shape = (B, 3, S, S)

    def losses(gd, net, pre, coin):
        R.random = (lambda: 0.0) if coin else (lambda: 1.0)  # the coin of ddpm.py:902
        for p in net.parameters():
            p.grad = None
        loss = gd.p_losses(x0, t, noise.clone())
        loss.backward()
        fx[pre + "loss"] = loss.detach().numpy()
        named = dict(net.named_parameters())
        for n in GNAMES:
            flat = named[n].grad.reshape(-1)
            if flat.numel() <= WHOLE:
                fx[pre + "grad:" + n] = named[n].grad.numpy().copy()
            else:
                fx[pre + "gradnorm:" + n] = np.float64(flat.double().norm().item())
                fx[pre + "gradsample:" + n] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[pre + "gradnorm_all"] = np.float64(
            torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item())
        return float(loss.detach())

    def ancestral64(gd64, init, nz):
        x, xs = init.double(), None
        for i, ti in enumerate(reversed(range(gd64.num_timesteps))):
            tb = torch.full((B,), ti, dtype=torch.long)
            mean, _, logvar, xs = gd64.p_mean_variance(x, tb, xs, clip_denoised=True)
            x = mean + (0.5 * logvar).exp() * nz[i].double() if ti > 0 else mean
        return (x + 1) * 0.5

    def ddim64(gd64, init, nz, eta):
        x, xs = init.double(), None
        for i, (ti, tn) in enumerate(O.ddim_time_pairs(gd64.num_timesteps, DDIM_STEPS)):
            tb = torch.full((B,), ti, dtype=torch.long)
            pn, xs = gd64.model_predictions(x, tb, xs, clip_x_start=True, rederive_pred_noise=True)
            if tn < 0:
                x = xs
                continue
            a, an = gd64.alphas_cumprod[ti], gd64.alphas_cumprod[tn]
            sigma = eta * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
            c = (1 - an - sigma ** 2).sqrt()
            x = xs * an.sqrt() + c * pn + sigma * nz[i].double()
        return (x + 1) * 0.5

    for o in OBJECTIVES:
        mk = lambda net, **kw: R.GaussianDiffusion(net, img_size=S, objective=o, **kw)  # noqa: E731
        gd = mk(unet, timesteps=1000, sampling_timesteps=DDIM_STEPS)
        gd64 = mk(unet64, timesteps=1000, sampling_timesteps=DDIM_STEPS).double()
        assert gd.self_condition
        x_t = gd.q_sample(x0, t, noise)
        fx[f"{o}:x_t"] = x_t.numpy()
        with torch.no_grad():
            fx[f"{o}:unet_out:sc"] = unet(x_t, t, sc).numpy()
            fx[f"{o}:unet_out:none"] = unet(x_t, t).numpy()
        l0 = losses(gd, unet, f"{o}:coin0:", False)
        l1 = losses(gd, unet, f"{o}:coin1:", True)
        with torch.no_grad():
            for clip in (False, True):
                pn, xs = gd.model_predictions(x_t, t, sc, clip_x_start=clip)
                fx[f"{o}:mp:{int(clip)}:pred_noise"] = pn.numpy().copy()
                fx[f"{o}:mp:{int(clip)}:x_start"] = xs.numpy().copy()
            fx[f"{o}:mp:0:x_start64"] = gd64.model_predictions(x_t.double(), t, sc.double()).pred_x_start.numpy().copy()
            torch.manual_seed(DDIM_SEED)
            fx[f"{o}:ddim_loop"] = gd.ddim_sample(shape).numpy()
            init, nz = O.draw_loop_noise(DDIM_SEED, shape, DDIM_STEPS - 1)
            fx[f"{o}:ddim_loop64"] = ddim64(gd64, init, nz, 0.0).numpy()
            gd_e = mk(unet, timesteps=1000, sampling_timesteps=DDIM_STEPS, ddim_sampling_eta=ETA)
            torch.manual_seed(DDIM_ETA_SEED)
            fx[f"{o}:ddim_eta_loop"] = gd_e.ddim_sample(shape).numpy()
            init, nz = O.draw_loop_noise(DDIM_ETA_SEED, shape, DDIM_STEPS - 1)
            fx[f"{o}:ddim_eta_loop64"] = ddim64(gd64, init, nz, ETA).numpy()
            gd_a = mk(unet, timesteps=ANCESTRAL_T)
            gd_a64 = mk(unet64, timesteps=ANCESTRAL_T).double()
            torch.manual_seed(ANCESTRAL_SEED)
            fx[f"{o}:p_sample_loop"] = gd_a.p_sample_loop(shape).numpy()
            init, nz = O.draw_loop_noise(ANCESTRAL_SEED, shape, ANCESTRAL_T - 1)
            fx[f"{o}:p_sample_loop64"] = ancestral64(gd_a64, init, nz).numpy()
        print(f"{o}: loss coin off {l0:.6f}  coin on {l1:.6f}")

    # one channel: the input buffer has a pitch of 4, the self-conditioning slice is lane 0 and the x slice lane 1
    P1 = O.unet_init(dim=dim, channels=1, seed=2)
    P1["init_conv.weight"] = _init_weight(dim, 2, C1_SEED)
    fx["c1:init_conv.weight"] = P1["init_conv.weight"].numpy()
    unet1 = R.Unet(dim=dim, channels=1, self_condition=True)
    unet1.load_state_dict(P1, strict=True)
    gd1 = R.GaussianDiffusion(unet1, img_size=S, timesteps=1000, objective="pred_v")
    x01, n1, sc1 = x0[:, :1].contiguous(), noise[:, :1].contiguous(), sc[:, :1].contiguous()
    with torch.no_grad():
        fx["c1:unet_out:sc"] = unet1(gd1.q_sample(x01, t, n1), t, sc1).numpy()
    R.random = lambda: 0.0
    fx["c1:coin1:loss"] = gd1.p_losses(x01, t, n1.clone()).detach().numpy()
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
