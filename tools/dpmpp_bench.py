"""Time DPM-Solver++ sampling beside DDIM on one GPU: ms per graph-replayed step of each (250-step chains, so the per-chain
setup is spread alike), and the wall time of a 20-step DPM-Solver++ chain beside the 250-step DDIM chain it replaces - 64 images
at 64 x 64 on the DDPM UNet (dim 64, random weights), every figure the median of three chains after one warm-up chain (which
also captures the step's graph).  The DDIM path is the one the parent commit has: this change does not touch it.

Usage:  python tools/dpmpp_bench.py [--out profiles/r10_dpmpp_bench.json] [--batch 64] [--size 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lightning-generative-models_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_dpmpp_bench.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--chains", type=int, default=3)
    a = ap.parse_args()
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = Unet(dim=64, channels=3)
    shape = (a.batch, 3, a.size, a.size)
    mk = lambda **kw: GaussianDiffusion(net, img_size=a.size, timesteps=1000, **kw).to(dev)  # noqa: E731
    runs = {"ddim_250": (mk(sampling_timesteps=250), sampler.ddim_sample, 250),
            "dpmpp_2m_250": (mk(sampling_timesteps=250, sampler="dpm++"), sampler.dpm_solver_sample, 250),
            "dpmpp_2m_20": (mk(sampling_timesteps=20, sampler="dpm++"), sampler.dpm_solver_sample, 20),
            "dpmpp_2m_sde_20": (mk(sampling_timesteps=20, sampler="dpm++", dpm_stochastic=True), sampler.dpm_solver_sample, 20)}
    net.prepare_hip(dev)
    init = torch.randn(shape, device=dev)
    out = {"what": f"{a.batch} images at {a.size} x {a.size}, DDPM UNet dim 64, one GPU; wall time of whole graph-replayed chains "
                   f"(torch.cuda.synchronize on both sides), median of {a.chains} after one warm-up chain; the DDIM path is "
                   "unchanged from the parent commit", "device": torch.cuda.get_device_name(0), "chains_ms": {}, "ms_per_step": {}}
    for name, (gd, fn, steps) in runs.items():
        img = fn(gd, shape, init_noise=init)                   # warm-up: capture + one chain
        assert torch.isfinite(img).all(), name
        graphed = any(isinstance(e, sampler._GraphedChain) for e in sampler._GRAPHS.get(net, {}).values())
        assert graphed, "graph replay is unavailable: the figures would be eager launches"
        times = []
        for _ in range(a.chains):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(gd, shape, init_noise=init)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out["chains_ms"][name] = [round(t, 3) for t in times]
        out["ms_per_step"][name] = round(statistics.median(times) / steps, 4)
        print(name, out["chains_ms"][name], out["ms_per_step"][name], flush=True)
    d, p = out["ms_per_step"]["ddim_250"], out["ms_per_step"]["dpmpp_2m_250"]
    out["dpmpp_step_over_ddim_step"] = round(p / d, 4)
    out["chain_20_step_dpmpp_over_250_step_ddim"] = round(statistics.median(out["chains_ms"]["dpmpp_2m_20"])
                                                          / statistics.median(out["chains_ms"]["ddim_250"]), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
