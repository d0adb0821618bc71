"""Time the variational-bound evaluation (``GaussianDiffusion.vlb_terms``) beside sampling on one GPU: ms per graph-replayed
evaluated term of a 20-timestep evaluation of 64 images at 64 x 64 on the DDPM UNet (dim 64, random weights), beside the ms per
step of a 20-step DDIM chain (eta 0) and a 20-step DPM-Solver++(2M) chain on the same network, the three alternating inside
one process; every figure is the median over ``--runs`` whole calls (``torch.cuda.synchronize`` on both sides) after one
warm-up call each, which also captures the step's graph.  An evaluated term is the DDIM step's forward plus three small
launches - the noise draw, q_sample and the reducer - in place of the update; each of the three is timed alone (device events
around back-to-back launches on the evaluation's own buffers), and so is the reducer (``lgm_vlb_term``, a KL row and the
decoder row) at 64 x 64 (B = 64), 128 x 128 and 256 x 256 (B = 8): one workgroup per sample.

``accepted``: a term costs no more than the DDIM step + the three launches alone, plus the 2 % between devices.

``--sampling-only`` times the two sampling chains alone and needs nothing of the evaluation; with ``--tree DIR`` it runs on
another checkout (the parent commit, with its own library) and ``--parent FILE ...`` puts the figures of such runs beside this
commit's; ``--attach KEY=FILE ...`` records the headline of other runs of the same call (``bench.py`` on both trees).

Usage:  python tools/bpd_bench.py [--out profiles/r13_bpd_bench.json] [--parent parent.json ...] [--sampling-only] [--tree DIR]
        [--attach KEY=FILE ...] [--base FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--tree", default=here, help="the checkout to import the package (and its library) from")
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r13_bpd_bench.json"))
    ap.add_argument("--parent", default=None, nargs="*", help="files --sampling-only runs on the parent commit wrote")
    ap.add_argument("--sampling-only", action="store_true")
    ap.add_argument("--attach", default=[], nargs="*", metavar="KEY=FILE",
                    help="put the headline of FILE (a JSON file, or one whose last line is JSON) under KEY (other runs of the same call: bench.py on both trees)")
    ap.add_argument("--base", default=None, help="measure nothing: start from this result file and apply --parent / --attach")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=15)
    a = ap.parse_args()
    out = json.load(open(a.base)) if a.base else measure(a, here)
    if a.parent:
        bases = [json.load(open(f)) for f in a.parent]
        out["parent_commit_ms_per_step"] = [b["ms_per_step"] for b in bases]
        for k in ("ddim_step", "dpmpp_step"):
            base = statistics.median(b["ms_per_step"][k] for b in bases)
            out[f"{k}_over_parent"] = round(out["ms_per_step"][k] / base, 4)
    for item in a.attach:
        key, path = item.split("=", 1)
        text = open(path).read().strip()
        try:
            rec = json.loads(text)                           # a result file of this tool
        except ValueError:
            rec = json.loads(text.splitlines()[-1])          # bench.py: one JSON line at the end
        out.setdefault("attached", {})[key] = {k: rec[k] for k in ("metric", "value", "ms_per_step") if k in rec}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def measure(a, here):
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops, sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    assert torch.cuda.is_available(), "bpd_bench needs a GPU: it does not fall back"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shape = (a.batch, 3, a.size, a.size)
    init = torch.randn(shape, device=dev)
    img = torch.rand(shape, device=dev)
    net = Unet(dim=64, channels=3)
    ddim = GaussianDiffusion(net, img_size=a.size, timesteps=1000, sampling_timesteps=a.steps).to(dev)
    dpm = GaussianDiffusion(net, img_size=a.size, timesteps=1000, sampling_timesteps=a.steps, sampler="dpm++").to(dev)
    net.prepare_hip(dev)
    times = [t for t, _ in ddim.ddim_time_pairs()]
    calls = {"ddim_step": lambda: sampler.ddim_sample(ddim, shape, init_noise=init),
             "dpmpp_step": lambda: sampler.dpm_solver_sample(dpm, shape, init_noise=init)}
    if not a.sampling_only:
        calls["bpd_term"] = lambda: ddim.vlb_terms(img, timesteps=times).vb
    out = {"what": f"{a.batch} images at {a.size} x {a.size}, DDPM UNet dim 64, one GPU, {a.steps} steps / evaluated timesteps per "
                   f"call, graph replay; wall time of whole calls (torch.cuda.synchronize on both sides) / {a.steps}, median of "
                   f"{a.runs} calls after one warm-up call, the kinds alternating",
           "device": torch.cuda.get_device_name(0), "tree": "this commit" if root == here else "parent commit",
           "ms_per_step": {}, "calls_ms": {}}
    for k, fn in calls.items():
        assert torch.isfinite(fn()).all(), k                         # warm-up: capture + one call
    graphs = [e for e in sampler._GRAPHS.get(net, {}).values() if not isinstance(e, int)]
    assert len(graphs) == len(calls), "graph replay is unavailable: the figures would be eager launches"
    wall = {k: [] for k in calls}
    for _ in range(a.runs):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    for k in calls:
        out["calls_ms"][k] = [round(t, 3) for t in wall[k]]
        out["ms_per_step"][k] = round(statistics.median(wall[k]) / a.steps, 4)
        print(k, out["ms_per_step"][k], flush=True)

    def alone(fn, n=200):
        """us per launch: n back-to-back launches between two device events, after 10 to warm up"""
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / n, 3)

    if not a.sampling_only:
        from lgm_hip import likelihood as LK
        rows = LK.vlb_plan(ddim, [500, 0])
        # the three launches an evaluated term adds, on the buffers of a term in mid-flight
        nz = torch.randn(shape, device=dev)
        xin = torch.zeros((a.batch, a.size, a.size, net.in_pitch), device=dev)
        tb = torch.full((a.batch,), 500, device=dev, dtype=torch.long)
        q = lambda: LK._qsample(ddim, img, nz, tb, ddim.sqrt_alphas_cumprod, ddim.sqrt_one_minus_alphas_cumprod, xin)  # noqa: E731
        q()
        v = net.forward_guided(xin, tb, None, 1.0)
        res = torch.zeros((1, 3, a.batch), device=dev)
        us = {"noise_draw": alone(lambda: torch.randn(shape, device=dev)), "q_sample": alone(q),
              "reducer_kl": alone(lambda: LK._launch_term(ddim, img, nz, xin, v, True, res, row=rows[0], at=0))}
        assert ops.lib()._dll.lgm_last_kernel().decode() == "vlb_term_kernel"
        us["reducer_decoder"] = alone(lambda: LK._launch_term(ddim, img, nz, xin, v, True, res, row=rows[1], at=0))
        out["launch_alone_us"] = us
        added = (us["noise_draw"] + us["q_sample"] + us["reducer_kl"]) * 1e-3
        d, t = out["ms_per_step"]["ddim_step"], out["ms_per_step"]["bpd_term"]
        out["bpd_term_minus_ddim_step_us"] = round((t - d) * 1e3, 2)
        out["bpd_term_bound_ms"] = round((d + added) * 1.02, 4)
        out["accepted"] = bool(t <= (d + added) * 1.02)
        # the reducer alone at three image sizes: one workgroup of 256 lanes per sample
        sizes = {}
        for B, S in ((64, 64), (8, 128), (8, 256)):
            g = torch.Generator(device=dev).manual_seed(S)
            im, z = torch.rand((B, 3, S * S), device=dev, generator=g), torch.randn((B, 3, S * S), device=dev, generator=g)
            xi, vv = torch.randn((B, S * S, 4), device=dev, generator=g), torch.randn((B, S * S, 4), device=dev, generator=g)
            o = torch.zeros((1, 3, B), device=dev)
            for name, row in (("kl", rows[0]), ("decoder", rows[1])):
                fn = lambda: ops.lib().lgm_vlb_term(im.data_ptr(), z.data_ptr(), 1, xi.data_ptr(), 4, 0, vv.data_ptr(), 4, B, 3,  # noqa: E731
                                                    S * S, 2, 1, *LK._byval(row), o.data_ptr(), 1, 0, ops.stream())
                sizes[f"B{B}_{S}x{S}_{name}"] = alone(fn)
            assert torch.isfinite(o).all()
        out["reducer_alone_us"] = sizes
        print(json.dumps({k: out[k] for k in ("launch_alone_us", "reducer_alone_us", "accepted")}), flush=True)
    return out


if __name__ == "__main__":
    main()
