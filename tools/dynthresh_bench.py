"""Time dynamically thresholded DPM-Solver++ sampling beside the static clamp on one GPU: ms per graph-replayed step of a
20-step chain of 64 images at 64 x 64 on the DDPM UNet (dim 64, random weights), unguided and guided at scale 3 (two forwards
and the mix per step), and the duration of the one launch thresholding adds (``lgm_dyn_thresh`` alone, device events around
back-to-back launches on the chain's own buffers).  Static and thresholded chains alternate inside one process; every chain
figure is the median over ``--chains`` chains after one warm-up chain each (which also captures the step's graph).

``--static-only`` runs on a tree without the feature: run it on the parent commit and hand the file it writes to ``--parent``
to put the baseline beside this commit's figures.

Usage:  python tools/dynthresh_bench.py [--out profiles/r11_dynthresh_bench.json] [--parent parent.json] [--static-only]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_dynthresh_bench.json"))
    ap.add_argument("--parent", default=None, help="the file a --static-only run on the parent commit wrote")
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chains", type=int, default=15)
    ap.add_argument("--scale", type=float, default=3.0)
    a = ap.parse_args()
    from lgm_hip import ops, sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shape = (a.batch, 3, a.size, a.size)
    init = torch.randn(shape, device=dev)
    out = {"what": f"{a.batch} images at {a.size} x {a.size}, DDPM UNet dim 64, one GPU, {a.steps}-step DPM-Solver++(2M) chains, graph "
                   f"replay; wall time of whole chains (torch.cuda.synchronize on both sides) / {a.steps}, median of {a.chains} "
                   "chains after one warm-up chain, static and thresholded chains alternating",
           "device": torch.cuda.get_device_name(0), "ms_per_step": {}, "chains_ms": {}}
    kinds = ("static",) if a.static_only else ("static", "thresholded")
    for config in ("unguided", "guided"):
        guided = config == "guided"
        net = Unet(dim=64, channels=3, **(dict(num_classes=10) if guided else {}))
        gds = {k: GaussianDiffusion(net, img_size=a.size, timesteps=1000, sampling_timesteps=a.steps, sampler="dpm++",
                                    **(dict(dynamic_thresholding=True) if k == "thresholded" else {})).to(dev) for k in kinds}
        net.prepare_hip(dev)
        y = (torch.arange(a.batch, device=dev) % 10) if guided else None
        scale = a.scale if guided else 1.0
        run = lambda gd: sampler.dpm_solver_sample(gd, shape, init_noise=init, classes=y, cond_scale=scale)  # noqa: E731
        for k in kinds:
            assert torch.isfinite(run(gds[k])).all(), (config, k)        # warm-up: capture + one chain
        entries = sampler._GRAPHS.get(net, {})
        assert len([e for e in entries.values() if isinstance(e, sampler._GraphedChain)]) == len(kinds), \
            "graph replay is unavailable: the figures would be eager launches"
        times = {k: [] for k in kinds}
        for _ in range(a.chains):
            for k in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(gds[k])
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        for k in kinds:
            out["chains_ms"][f"{config}_{k}"] = [round(t, 3) for t in times[k]]
            out["ms_per_step"][f"{config}_{k}"] = round(statistics.median(times[k]) / a.steps, 4)
            print(config, k, out["ms_per_step"][f"{config}_{k}"], flush=True)
        if not a.static_only and not guided:
            # the added launch alone, on the buffers of a chain in mid-flight (x and the network output of a real step)
            gd = gds["thresholded"]
            chain = sampler._Chain(gd, shape, init)
            pairs = gd.dpm_time_pairs()
            rows = sampler.dpm_coeffs(gd, pairs, gd.dpm_order, gd.dpm_stochastic)
            for (t, _), row in list(zip(pairs, rows))[:3]:
                sampler.dpm_step(chain, t, None, row)
            v = net.forward_guided(chain.x, chain.times(pairs[3][0]), None, 1.0)
            head = rows[3][:4]
            n = 200
            for _ in range(10):
                chain._dyn_thresh(v, head)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                chain._dyn_thresh(v, head)
            e1.record()
            torch.cuda.synchronize()
            assert ops.lib()._dll.lgm_last_kernel().decode() == "dyn_thresh_kernel"
            out["dyn_thresh_launch_us"] = round(e0.elapsed_time(e1) * 1e3 / n, 3)
            out["dyn_thresh_launch_what"] = (f"lgm_dyn_thresh alone, {n} back-to-back launches between two device events: "
                                             f"{a.batch} workgroups of 1024 threads, {3 * a.size * a.size} values each, "
                                             "thresholds of that step " + str([round(float(s), 3) for s in chain.thresh[:4]]))
            print("dyn_thresh launch, us:", out["dyn_thresh_launch_us"], flush=True)
    if not a.static_only:
        for config in ("unguided", "guided"):
            s, t = out["ms_per_step"][f"{config}_static"], out["ms_per_step"][f"{config}_thresholded"]
            out[f"{config}_step_delta_us"] = round((t - s) * 1e3, 2)
            out[f"{config}_thresholded_over_static"] = round(t / s, 4)
    if a.parent:
        base = json.load(open(a.parent))
        out["parent_commit_static_ms_per_step"] = {k: v for k, v in base["ms_per_step"].items()}
        for config in ("unguided", "guided"):
            out[f"{config}_static_over_parent"] = round(out["ms_per_step"][f"{config}_static"]
                                                        / base["ms_per_step"][f"{config}_static"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
