"""Generate tests/golden/diffusion_classcond.npz: the REAL reference's ``Unet`` / ``GaussianDiffusion`` on CPU with a label
embedding added to the time embedding and classifier-free guidance, for ``objective="pred_v"`` and ``"pred_noise"``.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_selfcond.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_classcond.py [--check]

The reference has no class conditioning; two thin wrappers of this file put it around the reference's own arithmetic.
``_TimePlusLabel`` takes the place of ``Unet.time_mlp`` (an ``nn.Sequential`` attribute) and returns
``time_mlp(t) + label_emb[classes]``; ``_Guided`` takes the place of the network inside ``GaussianDiffusion`` and returns
``out_null + cond_scale * (out_cond - out_null)`` (one forward when the scale is 1).  The reference's ``p_losses``,
``model_predictions``, ``p_sample_loop`` and ``ddim_sample`` then run unchanged.

The recipe is the "small" network (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16) with K = 5 classes, B = 4,
classes = (3, 0, 3, 5) - class 3 twice: a two-term sum; rows 1, 2 and 4 absent: exactly zero gradient; 5 = the null label -
t = (37, 912, 0, 999), data seed 101 and a seeded [6, 64] embedding stored in the file.  Stored per objective: the UNet
output with the labels and with all-null labels; p_losses' loss and gradients (label_emb.weight whole, the others as GNAMES:
whole up to 8192 elements, else norm + strided sample); model_predictions at cond_scale 1 and 3, clip off and on; a 50-step
ancestral chain (timesteps=50) and a 20-pair DDIM chain (eta = 0 and 0.7) at cond_scale 3 (the tests replay the draws with
oracle.diffusion.draw_loop_noise), and for every chain and for the unclipped x_start a float64 evaluation of the same
modules for the arbiter.  One self-conditioned + class-conditional case (pred_v): output and loss, coin on.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_classcond.npz")

from tools.make_golden_objectives import GNAMES, SAMPLE, WHOLE  # noqa: E402
from tools.make_golden_selfcond import INIT_W_SEED, SC_SEED, _init_weight  # noqa: E402

OBJECTIVES = ("pred_v", "pred_noise")
K, CLASSES, TIMES = 5, (3, 0, 3, 5), (37, 912, 0, 999)
EMB_SEED, SCALE = 711, 3.0
DDIM_SEED, ANCESTRAL_SEED, DDIM_ETA_SEED, ETA = 9101, 9102, 9103, 0.7
DDIM_STEPS, ANCESTRAL_T = 20, 50


class _TimePlusLabel(nn.Module):
    """in place of ``Unet.time_mlp``: the time embedding plus one row of the label embedding per sample"""

    def __init__(self, time_mlp, weight):
        super().__init__()
        self.time_mlp = time_mlp
        self.weight = nn.Parameter(weight.clone())
        self.classes = None

    def forward(self, t):
        return self.time_mlp(t) + self.weight[self.classes]


class _Guided(nn.Module):
    """in place of the network inside GaussianDiffusion: conditional forward, null-label forward, their mix"""

    def __init__(self, unet, classes, scale):
        super().__init__()
        self.unet, self.classes, self.scale = unet, torch.as_tensor(classes), float(scale)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__("unet"), name)

    def forward(self, x, t, x_self_cond=None):
        emb = self.unet.time_mlp
        emb.classes = self.classes
        cond = self.unet(x, t, x_self_cond)
        if self.scale == 1.0:
            return cond
        emb.classes = torch.full_like(self.classes, K)
        null = self.unet(x, t, x_self_cond)
        return null + self.scale * (cond - null)


def _pname(n):
    """parameter name of the wrapped network -> name in a Unet(num_classes=K)"""
    if n == "time_mlp.weight":
        return "label_emb.weight"
    return n.replace("time_mlp.time_mlp.", "time_mlp.")


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, len(CLASSES), 1
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "K": K, "data_seed": 100 + seed, "cond_scale": np.float32(SCALE),
          "ddim_loop_seed": DDIM_SEED, "p_sample_loop_seed": ANCESTRAL_SEED, "ddim_eta_loop_seed": DDIM_ETA_SEED,
          "eta": np.float32(ETA), "ddim_steps": DDIM_STEPS, "ancestral_T": ANCESTRAL_T, "grad_sample": SAMPLE}
    classes, t = torch.tensor(CLASSES), torch.tensor(TIMES)
    fx["classes"], fx["t"] = classes.numpy(), t.numpy()
    emb = torch.randn(K + 1, 4 * dim, generator=torch.Generator().manual_seed(EMB_SEED))
    fx["label_emb.weight"] = emb.numpy()
    P = O.unet_init(dim=dim, channels=3, seed=seed)

    def network(self_condition=False, double=False):
        net = R.Unet(dim=dim, channels=3, self_condition=self_condition)
        Pn = dict(P)
        if self_condition:
            Pn["init_conv.weight"] = _init_weight(dim, 6, INIT_W_SEED)
        net.load_state_dict(Pn, strict=True)
        names = list(net.state_dict().keys())
        net.time_mlp = _TimePlusLabel(net.time_mlp, emb)
        if double:
            net.double()
            # the time embedding takes its dtype from ``time``: hand the float64 network float64 timesteps
            net.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
        return net, names

    unet, names = network()
    unet64, _ = network(double=True)
    at = names.index("time_mlp.3.bias") + 1
    sd = {_pname(k): v for k, v in unet.state_dict().items()}
    order = names[:at] + ["label_emb.weight"] + names[at:]
    fx["sd_names"] = np.asarray(order)
    fx["sd_shapes"] = np.asarray([list(sd[n].shape) + [0] * (4 - sd[n].dim()) for n in order], dtype=np.int64)
    g = torch.Generator().manual_seed(100 + seed)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)
    x0 = img * 2 - 1
    shape = (B, 3, S, S)
    null = torch.full_like(classes, K)

    def ancestral64(gd64, init, nz):
        x = init.double()
        for i, ti in enumerate(reversed(range(gd64.num_timesteps))):
            tb = torch.full((B,), ti, dtype=torch.long)
            mean, _, logvar, _ = gd64.p_mean_variance(x, tb, None, clip_denoised=True)
            x = mean + (0.5 * logvar).exp() * nz[i].double() if ti > 0 else mean
        return (x + 1) * 0.5

    def ddim64(gd64, init, nz, eta):
        x = init.double()
        for i, (ti, tn) in enumerate(O.ddim_time_pairs(gd64.num_timesteps, DDIM_STEPS)):
            tb = torch.full((B,), ti, dtype=torch.long)
            pn, xs = gd64.model_predictions(x, tb, None, clip_x_start=True, rederive_pred_noise=True)
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
        gd = mk(unet, timesteps=1000)
        x_t = gd.q_sample(x0, t, noise)
        fx[f"{o}:x_t"] = x_t.numpy()
        with torch.no_grad():
            fx[f"{o}:unet_out:cond"] = _Guided(unet, classes, 1.0)(x_t, t).numpy()
            fx[f"{o}:unet_out:null"] = _Guided(unet, null, 1.0)(x_t, t).numpy()
        # the training step: the labels as given (already dropped: sample 3 carries the null label)
        unet.time_mlp.classes = classes
        for p in unet.parameters():
            p.grad = None
        loss = gd.p_losses(x0, t, noise.clone())
        loss.backward()
        fx[f"{o}:loss"] = loss.detach().numpy()
        named = {_pname(n): p for n, p in unet.named_parameters()}
        fx[f"{o}:grad:label_emb.weight"] = named["label_emb.weight"].grad.numpy().copy()
        for n in GNAMES:
            flat = named[n].grad.reshape(-1)
            if flat.numel() <= WHOLE:
                fx[f"{o}:grad:{n}"] = named[n].grad.numpy().copy()
            else:
                fx[f"{o}:gradnorm:{n}"] = np.float64(flat.double().norm().item())
                fx[f"{o}:gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[f"{o}:gradnorm_all"] = np.float64(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in unet.parameters())).item())
        with torch.no_grad():
            for scale in (1.0, SCALE):
                gds = mk(_Guided(unet, classes, scale), timesteps=1000)
                gds64 = mk(_Guided(unet64, classes, scale), timesteps=1000).double()
                for clip in (False, True):
                    pn, xs = gds.model_predictions(x_t, t, None, clip_x_start=clip)
                    fx[f"{o}:mp:s{int(scale)}:{int(clip)}:pred_noise"] = pn.numpy().copy()
                    fx[f"{o}:mp:s{int(scale)}:{int(clip)}:x_start"] = xs.numpy().copy()
                fx[f"{o}:mp:s{int(scale)}:0:x_start64"] = gds64.model_predictions(x_t.double(), t).pred_x_start.numpy().copy()
            net3, net3_64 = _Guided(unet, classes, SCALE), _Guided(unet64, classes, SCALE)
            gd_d = mk(net3, timesteps=1000, sampling_timesteps=DDIM_STEPS)
            gd_d64 = mk(net3_64, timesteps=1000, sampling_timesteps=DDIM_STEPS).double()
            torch.manual_seed(DDIM_SEED)
            fx[f"{o}:ddim_loop"] = gd_d.ddim_sample(shape).numpy()
            init, nz = O.draw_loop_noise(DDIM_SEED, shape, DDIM_STEPS - 1)
            fx[f"{o}:ddim_loop64"] = ddim64(gd_d64, init, nz, 0.0).numpy()
            gd_e = mk(net3, timesteps=1000, sampling_timesteps=DDIM_STEPS, ddim_sampling_eta=ETA)
            torch.manual_seed(DDIM_ETA_SEED)
            fx[f"{o}:ddim_eta_loop"] = gd_e.ddim_sample(shape).numpy()
            init, nz = O.draw_loop_noise(DDIM_ETA_SEED, shape, DDIM_STEPS - 1)
            fx[f"{o}:ddim_eta_loop64"] = ddim64(gd_d64, init, nz, ETA).numpy()
            gd_a = mk(net3, timesteps=ANCESTRAL_T)
            gd_a64 = mk(net3_64, timesteps=ANCESTRAL_T).double()
            torch.manual_seed(ANCESTRAL_SEED)
            fx[f"{o}:p_sample_loop"] = gd_a.p_sample_loop(shape).numpy()
            init, nz = O.draw_loop_noise(ANCESTRAL_SEED, shape, ANCESTRAL_T - 1)
            fx[f"{o}:p_sample_loop64"] = ancestral64(gd_a64, init, nz).numpy()
        print(f"{o}: loss {float(loss.detach()):.6f}")

    # self-conditioned + class-conditional (pred_v): the estimate pass and the main pass see the same labels
    unet_sc, _ = network(self_condition=True)
    fx["sc:init_conv.weight"] = unet_sc.init_conv.weight.detach().numpy().copy()
    sc = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(SC_SEED)) * 2 - 1
    fx["sc:x_self_cond"] = sc.numpy()
    gd_sc = R.GaussianDiffusion(unet_sc, img_size=S, timesteps=1000, objective="pred_v")
    unet_sc.time_mlp.classes = classes
    with torch.no_grad():
        fx["sc:unet_out"] = unet_sc(gd_sc.q_sample(x0, t, noise), t, sc).numpy()
    R.random = lambda: 0.0                                   # the reference's coin (random() < 0.5): on
    fx["sc:coin1:loss"] = gd_sc.p_losses(x0, t, noise.clone()).detach().numpy()
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
