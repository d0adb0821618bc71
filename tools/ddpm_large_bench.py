"""The DDPM UNet (dim 64) at 128 x 128 and 256 x 256 on one GPU: one JSON line per leg.

Legs (``--legs``, comma-separated, default all):
  train128     training step (forward + backward + Adam + EMA, DDPMFastStep graph replay), 128 x 128, B = 32
  train256     the same at 256 x 256, B = 8
  ddim128      one DDIM step (UNet forward + update, one graph replay per step), 128 x 128, B = 16
  torch128     the train128 step as eager PyTorch-ROCm ops over oracle.diffusion (+ torch.optim.Adam) on the same GPU
  attn         isolated full attention forward + backward at n = 256 (B = 32) and n = 1024 (B = 8), heads 4, M 4

Training legs are timed as bench.py times its DDPM legs: warm-up steps (the first captures the graphs), synchronize,
``--steps`` timed steps, synchronize.  python tools/ddpm_large_bench.py [--steps K] [--warmup W] [--legs a,b]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lightning-generative-models_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def _timed(one, warmup, steps):
    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(warmup + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def train_leg(dev, img, batch, warmup, steps):
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    model = DDPM(img_channels=3, img_size=img, dim=64, diffusion_timesteps=1000, sampling_timesteps=None,
                 lr=2e-5, betas=(0.9, 0.99), ema_update_every=10, ema_decay=0.995)
    model.sample_every = 0
    model.to(dev)
    model.prepare_hip(dev)
    model.train()
    opt = model.configure_optimizers()
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(batch, 3, img, img, generator=g) * 2 - 1).to(dev)
    y = torch.zeros(batch, dtype=torch.long, device=dev)
    fast = DDPMFastStep(model, opt, 1, use_graph=True)
    losses = []
    dt = _timed(lambda i: losses.append(fast.step((x, y), i)), warmup, steps)
    return {"leg": f"train{img}", "metric": f"DDPM training step {img}x{img}, B={batch} (graph replay)",
            "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(batch / dt, 2),
            "finite": bool(torch.isfinite(torch.stack([l.reshape(()) for l in losses])).all()),
            "config": {"img": img, "batch": batch, "warmup": warmup, "steps": steps}}


def ddim_leg(dev, img, batch, steps):
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(img_channels=3, img_size=img, dim=64, diffusion_timesteps=1000, sampling_timesteps=steps).to(dev)
    m.sample_every = 0
    m.prepare_hip(dev)
    gd = m.ema.ema_model
    gd.eval()
    shape = (batch, 3, img, img)
    sampler.ddim_sample(gd, shape)                   # capture + one whole chain as warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sampler.ddim_sample(gd, shape)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"leg": f"ddim{img}", "metric": f"one DDIM step {img}x{img}, B={batch} (mean over a {steps}-step chain)",
            "ms_per_step": round(dt * 1e3, 3), "image_steps_per_s": round(batch / dt, 1),
            "finite": bool(torch.isfinite(out).all()), "config": {"img": img, "batch": batch, "steps": steps}}


def torch_leg(dev, img, batch, warmup, steps):
    from oracle import diffusion as OD
    torch.manual_seed(10)
    P = {k: v.to(dev).requires_grad_(True) for k, v in OD.unet_init(dim=64, channels=3, seed=0).items()}
    bufs = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in OD.diffusion_buffers(1000).items()}
    opt = torch.optim.Adam(list(P.values()), lr=2e-5, betas=(0.9, 0.99))
    x = (torch.rand(batch, 3, img, img) * 2 - 1).to(dev)

    def one(i):
        t = torch.randint(0, 1000, (batch,), device=dev)
        loss = OD.diffusion_forward(P, bufs, x, t, torch.randn_like(x), dim=64)
        opt.zero_grad()
        loss.backward()
        opt.step()

    dt = _timed(one, warmup, steps)
    return {"leg": f"torch{img}", "metric": f"eager PyTorch-ROCm oracle.diffusion training step {img}x{img}, B={batch}",
            "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(batch / dt, 2),
            "config": {"img": img, "batch": batch, "warmup": warmup, "steps": steps}}


def attn_leg(dev, n_side, batch, iters=50, heads=4, M=4):
    from lgm_hip import ops
    d, hidden = 32, heads * 32
    g = torch.Generator().manual_seed(n_side)
    qkv = torch.randn(batch, n_side, n_side, 3 * hidden, generator=g).to(dev)
    gout = torch.randn(batch, n_side, n_side, hidden, generator=g).to(dev)
    mem = torch.randn(2 * heads * M * d, generator=g).to(dev)
    out = torch.empty(batch, n_side, n_side, hidden, device=dev)
    gq = torch.empty_like(qkv)
    gm = torch.zeros_like(mem)
    res = {}

    def fwd(i):
        res["lse"] = ops.attn_fwd(qkv, mem.data_ptr(), heads, d, M, out)

    def bwd(i):
        ops.attn_bwd(qkv, mem.data_ptr(), out, gout, res["lse"], heads, d, M, gq, gm.data_ptr(), 0.0)

    tf = _timed(fwd, 5, iters)
    tb = _timed(bwd, 5, iters)
    n = n_side * n_side
    flop_f = 4.0 * batch * heads * n * (n + M) * d
    return {"leg": f"attn_n{n}", "metric": f"full attention fwd + bwd, n={n}, B={batch}, heads={heads}, M={M}",
            "fwd_us": round(tf * 1e6, 1), "bwd_us": round(tb * 1e6, 1),
            "fwd_tflops": round(flop_f / tf / 1e12, 2), "bwd_tflops": round(2.5 * flop_f / tb / 1e12, 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--legs", default="train128,train256,ddim128,torch128,attn")
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    legs = a.legs.split(",")
    results = {}
    for leg in legs:
        if leg == "train128":
            r = train_leg(dev, 128, 32, a.warmup, a.steps)
        elif leg == "train256":
            r = train_leg(dev, 256, 8, a.warmup, a.steps)
        elif leg == "ddim128":
            r = ddim_leg(dev, 128, 16, max(a.steps, 10))
        elif leg == "torch128":
            r = torch_leg(dev, 128, 32, a.warmup, a.steps)
        elif leg == "attn":
            for n_side, b in ((16, 32), (32, 8)):
                print(json.dumps(attn_leg(dev, n_side, b)), flush=True)
            continue
        else:
            raise SystemExit(f"unknown leg {leg}")
        results[leg] = r
        if leg == "torch128" and "train128" in results:
            r["hip_speedup"] = round(r["ms_per_step"] / results["train128"]["ms_per_step"], 2)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
