"""Time inpainting chains beside the plain chains of the same samplers on one GPU: ms per graph-replayed step (one UNet forward
and one update launch) of 64 images at 64 x 64 on the DDPM UNet (dim 64, random weights), for the ancestral chain (a
``--ancestral-steps``-level diffusion) and DPM-Solver++(2M) (``--steps`` pairs).  The inpainting chain resamples (``--jump``,
``--resamples``), so it has more steps than the plain one; every figure is chain wall time / number of steps of that chain.
Plain and inpainting chains alternate inside one process; every figure is the median over ``--chains`` chains after one
warm-up chain each (which also captures the step's graph).

``--plain-only`` runs on a tree without the feature: run it on the parent commit and hand the file it writes to ``--parent``
to put the baseline beside this commit's figures.

Usage:  python tools/inpaint_bench.py [--out profiles/r12_inpaint_bench.json] [--parent parent.json] [--plain-only]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_inpaint_bench.json"))
    ap.add_argument("--parent", default=None, help="the file a --plain-only run on the parent commit wrote")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ancestral-steps", type=int, default=50)
    ap.add_argument("--jump", type=int, default=5)
    ap.add_argument("--resamples", type=int, default=2)
    ap.add_argument("--chains", type=int, default=15)
    a = ap.parse_args()
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shape = (a.batch, 3, a.size, a.size)
    init = torch.randn(shape, device=dev)
    known = torch.rand(shape, device=dev) * 2 - 1
    mask = torch.zeros(a.batch, 1, a.size, a.size, device=dev)
    mask[..., : a.size // 2] = 1.0
    out = {"what": f"{a.batch} images at {a.size} x {a.size}, DDPM UNet dim 64, one GPU, graph replay; wall time of whole chains "
                   f"(torch.cuda.synchronize on both sides) / steps of the chain, median of {a.chains} chains after one warm-up "
                   f"chain, plain and inpainting chains alternating; inpainting walks (jump_length, resamples) = ({a.jump}, "
                   f"{a.resamples}) with a half-image mask and draws on the device",
           "device": torch.cuda.get_device_name(0), "ms_per_step": {}, "steps": {}, "chains_ms": {}}
    kinds = ("plain",) if a.plain_only else ("plain", "inpaint")
    net = Unet(dim=64, channels=3)
    for config in ("ancestral", "dpm++"):
        if config == "ancestral":
            gd = GaussianDiffusion(net, img_size=a.size, timesteps=a.ancestral_steps).to(dev)
            plain = lambda: sampler.p_sample_loop(gd, shape, init_noise=init)  # noqa: E731
        else:
            gd = GaussianDiffusion(net, img_size=a.size, timesteps=1000, sampling_timesteps=a.steps, sampler="dpm++").to(dev)
            plain = lambda: sampler.dpm_solver_sample(gd, shape, init_noise=init)  # noqa: E731
        net.prepare_hip(dev)
        runs = {"plain": plain}
        steps = {"plain": a.ancestral_steps if config == "ancestral" else a.steps}
        if not a.plain_only:
            runs["inpaint"] = lambda: sampler.inpaint(gd, known, mask, a.jump, a.resamples, init_noise=init)  # noqa: E731
            steps["inpaint"] = len(sampler._plan_inpaint(gd, a.jump, a.resamples).times)
        before = len([e for e in sampler._GRAPHS.get(net, {}).values() if isinstance(e, sampler._GraphedChain)])
        for k in kinds:
            assert torch.isfinite(runs[k]()).all(), (config, k)          # warm-up: capture + one chain
        entries = sampler._GRAPHS.get(net, {})
        assert len([e for e in entries.values() if isinstance(e, sampler._GraphedChain)]) == before + len(kinds), \
            "graph replay is unavailable: the figures would be eager launches"
        times = {k: [] for k in kinds}
        for _ in range(a.chains):
            for k in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[k]()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        for k in kinds:
            out["steps"][f"{config}_{k}"] = steps[k]
            out["chains_ms"][f"{config}_{k}"] = [round(t, 3) for t in times[k]]
            out["ms_per_step"][f"{config}_{k}"] = round(statistics.median(times[k]) / steps[k], 4)
            print(config, k, steps[k], "steps,", out["ms_per_step"][f"{config}_{k}"], "ms per step", flush=True)
    if not a.plain_only:
        for config in ("ancestral", "dpm++"):
            s, t = out["ms_per_step"][f"{config}_plain"], out["ms_per_step"][f"{config}_inpaint"]
            out[f"{config}_step_delta_us"] = round((t - s) * 1e3, 2)
            out[f"{config}_inpaint_over_plain"] = round(t / s, 4)
    if a.parent:
        base = json.load(open(a.parent))
        out["parent_commit_plain_ms_per_step"] = {k: v for k, v in base["ms_per_step"].items()}
        for config in ("ancestral", "dpm++"):
            out[f"{config}_plain_over_parent"] = round(out["ms_per_step"][f"{config}_plain"]
                                                       / base["ms_per_step"][f"{config}_plain"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
