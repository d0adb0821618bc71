"""Generate tests/golden/diffusion_objectives.npz by running the REAL reference's GaussianDiffusion on CPU with
``objective="pred_noise"`` and ``"pred_x0"`` (and offset noise).

TEST INFRASTRUCTURE ONLY, like oracle/make_golden.py, whose import-time stubs and reference location it reuses: it runs
where the reference checkout is available and nowhere else.  Usage:  python tools/make_golden_objectives.py

The recipe is gen_diffusion's "small" case (oracle.unet_init(dim=16, channels=3, seed=1), 16 x 16, B = 2, t = (37, 912),
data seed 101), so the tests rebuild weights and inputs from seeds; only inputs the tests cannot re-draw and the reference's
outputs are stored, as float32 (checksums as float64).  Of the 26 named gradients the 23 with at most 8192 elements are
stored whole; the three large ones (downs.3.3.weight, mid_attn.to_qkv.weight, ups.0.0.res_conv.weight: 147 k elements
together, four times over) as their float64 norm and a 1024-element strided sample, the way gen_diffusion stores its
full-size cases: that keeps the file under the repository's limit for a committed file.

Re-running the script reproduces the file bit for bit on the same CPU, torch build and thread count (every draw is
seeded, the thread count is pinned, numpy stamps archive members with a fixed date).  Another host's CPU kernels sum in
another order: there the arrays behind the reference UNet's forward move by a few 1e-6 relative and the file differs,
while two runs on that host still agree with each other.  ``--check`` regenerates into a temporary file and compares it
with the committed one.
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
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_objectives.npz")

OBJECTIVES = ("pred_noise", "pred_x0")
GNAMES = ["init_conv.weight", "init_conv.bias", "time_mlp.1.weight", "time_mlp.3.bias",
          "downs.0.0.mlp.1.weight", "downs.0.0.block1.proj.weight", "downs.0.0.block1.norm.weight",
          "downs.0.0.block1.norm.bias", "downs.0.2.mem_kv", "downs.0.2.norm.g",
          "downs.0.2.to_qkv.weight", "downs.0.2.to_out.0.bias", "downs.0.2.to_out.1.g",
          "downs.0.3.1.weight", "downs.3.2.mem_kv", "downs.3.2.to_out.weight", "downs.3.3.weight",
          "mid_attn.to_qkv.weight", "mid_block1.block2.proj.bias", "ups.0.0.res_conv.weight",
          "ups.1.2.mem_kv", "ups.2.3.1.weight", "ups.3.3.bias", "final_res_block.res_conv.weight",
          "final_conv.weight", "final_conv.bias"]            # the 26 tensors of diffusion_unet_small.npz
OFFSET_SEED, OFFSET_STRENGTH = 4243, 0.1
WHOLE, SAMPLE = 8192, 1024        # gradients up to WHOLE elements are stored whole, larger ones as norm + SAMPLE elements


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B, seed = 16, 16, 2, 1
    fx = {"seed": seed, "dim": dim, "S": S, "B": B, "data_seed": 100 + seed, "offset_seed": OFFSET_SEED,
          "offset_strength": np.float32(OFFSET_STRENGTH)}
    idx = [0, 1, 2, 10, 100, 250, 500, 750, 900, 990, 998, 999]      # the indices of diffusion_schedule.npz
    fx["idx"] = np.asarray(idx)
    P = O.unet_init(dim=dim, channels=3, seed=seed)
    unet = R.Unet(dim=dim, channels=3)
    unet.load_state_dict(P, strict=True)
    g = torch.Generator().manual_seed(100 + seed)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)
    t = torch.tensor([37, 912])
    fx["t"] = t.numpy()
    x0 = img * 2 - 1

    # loss_weight (ddpm.py:649-662), all three objectives, with and without the min-SNR clamp (gamma = 5)
    for o in OBJECTIVES + ("pred_v",):
        for tag, on in (("", False), ("_minsnr", True)):
            lw = R.GaussianDiffusion(unet, img_size=S, timesteps=1000, objective=o, min_snr_loss_weight=on,
                                     min_snr_gamma=5).loss_weight
            fx[f"{o}:loss_weight{tag}"] = lw[idx].numpy()
            fx[f"{o}:loss_weight{tag}__sum"] = np.float64(lw.double().sum().item())

    def losses(gd, pre, **kw):
        for p in unet.parameters():
            p.grad = None
        loss = gd.p_losses(x0, t, noise.clone(), **kw)       # a clone: offset noise is added to the argument in place
        loss.backward()
        fx[pre + "loss"] = loss.detach().numpy()
        sd = dict(unet.named_parameters())
        for n in GNAMES:
            flat = sd[n].grad.reshape(-1)
            if flat.numel() <= WHOLE:
                fx[pre + "grad:" + n] = sd[n].grad.numpy().copy()
            else:
                fx[pre + "gradnorm:" + n] = np.float64(flat.double().norm().item())
                fx[pre + "gradsample:" + n] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[pre + "gradnorm_all"] = np.float64(
            torch.sqrt(sum(p.grad.double().pow(2).sum() for p in unet.parameters())).item())
        return float(loss.detach())

    for o in OBJECTIVES:
        gd = R.GaussianDiffusion(unet, img_size=S, timesteps=1000, sampling_timesteps=50, objective=o)
        x_t = gd.q_sample(x0, t, noise)
        fx[f"{o}:x_t"] = x_t.numpy()
        with torch.no_grad():
            fx[f"{o}:unet_out"] = unet(x_t, t).numpy()
        l0 = losses(gd, f"{o}:")
        # offset noise: p_losses draws randn([B, C]) from the global generator first thing (:890)
        torch.manual_seed(OFFSET_SEED)
        l1 = losses(gd, f"{o}:offset:", offset_noise_strength=OFFSET_STRENGTH)
        torch.manual_seed(OFFSET_SEED)
        off = torch.randn(B, 3)
        fx[f"{o}:offset_noise"] = off.numpy()
        x_to = gd.q_sample(x0, t, noise + OFFSET_STRENGTH * off[:, :, None, None])
        fx[f"{o}:offset:x_t"] = x_to.numpy()
        with torch.no_grad():
            fx[f"{o}:offset:unet_out"] = unet(x_to, t).numpy()
            for clip in (False, True):
                for red in (False, True):
                    pn, xs = gd.model_predictions(x_t, t, clip_x_start=clip, rederive_pred_noise=red)
                    fx[f"{o}:mp:{int(clip)}{int(red)}:pred_noise"] = pn.numpy().copy()
                    fx[f"{o}:mp:{int(clip)}{int(red)}:x_start"] = xs.numpy().copy()
            torch.manual_seed(4242)
            img_next, _ = gd.p_sample(x_t, 500)
            torch.manual_seed(4242)
            fx[f"{o}:p_sample_noise"] = torch.randn_like(x_t).numpy()
            fx[f"{o}:p_sample_500"] = img_next.numpy()
            fx[f"{o}:p_sample_0"] = gd.p_sample(x_t, 0)[0].numpy()
            tt = torch.full((B,), 999, dtype=torch.long)
            pn, xs = gd.model_predictions(x_t, tt, clip_x_start=True, rederive_pred_noise=True)
            a, an = gd.alphas_cumprod[999], gd.alphas_cumprod[979]
            sigma = 0.0 * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
            c = (1 - an - sigma ** 2).sqrt()
            fx[f"{o}:ddim_999_979"] = (xs * an.sqrt() + c * pn).numpy()
            torch.manual_seed(9001)
            fx[f"{o}:ddim_loop_50"] = gd.ddim_sample((B, 3, S, S)).numpy()
            gd_a = R.GaussianDiffusion(unet, img_size=S, timesteps=200, objective=o)
            torch.manual_seed(9002)
            fx[f"{o}:p_sample_loop_200"] = gd_a.p_sample_loop((B, 3, S, S)).numpy()
        print(f"{o}: loss {l0:.6f}  with offset noise {l1:.6f}  gradnorm {fx[o + ':gradnorm_all']:.6f}")
    fx["ddim_loop_seed"], fx["p_sample_loop_seed"], fx["grad_sample"] = 9001, 9002, SAMPLE
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
