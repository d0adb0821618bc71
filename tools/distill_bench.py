"""Measure what progressive distillation costs and what it saves -> profiles/r19_distill_bench.json.  Needs a GPU; nothing falls back.

  (i)   the plain step of THIS tree and of the parent commit's tree (``--parent-tree``, built), each in fresh processes,
        alternating: a model without a teacher adds no launch, so the two must sit inside the documented +-2 %;
  (ii)  the distilling step at 32 x 32, B = 128 beside the plain step, one process, graph replay, alternating windows;
  (iii) between device events: the teacher's two forwards without saved activations (eager launches) and the two new kernels
        alone, with their algorithmic bytes and achieved bandwidth beside ``qsample_slice_kernel``'s;
  (iv)  one sampled batch of 64 at 64 x 64: DDIM at N = 4 and 8 steps (what a distilled student runs) beside DDIM at 250 and
        DPM-Solver++ at 20.  TIME ONLY: the networks are untrained, sample quality at these step counts is not measured here.

Usage:  python tools/distill_bench.py [--parent-tree DIR] [--bench FILE ...] [--bench-parent FILE ...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--tree", default=here, help="the checkout to import the package (and its library) from")
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r19_distill_bench.json"))
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, built: (i) alternates with it")
    ap.add_argument("--plain-only", action="store_true", help="child mode: the plain step of --tree alone, JSON on stdout")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench", default=None, nargs="*", help="files holding bench.py's JSON result line, this commit")
    ap.add_argument("--bench-parent", default=None, nargs="*", help="the same from the parent commit's tree")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    a = ap.parse_args()
    if a.plain_only:
        print("RESULT " + json.dumps(measure(a, plain_only=True)))
        return
    out = {}
    if a.parent_tree:
        rounds = {"this commit": [], "parent commit": []}
        for _ in range(a.rounds):
            for name, tree in (("parent commit", a.parent_tree), ("this commit", here)):
                rounds[name].append(_child(a, tree)["plain_step_ms"])
        out["plain_32_step_ms_by_tree"] = rounds
        out["plain_32_step_over_parent"] = round(statistics.median(rounds["this commit"]) / statistics.median(rounds["parent commit"]), 4)
    out.update(measure(a, plain_only=False))
    for key, files in (("bench_py", a.bench), ("bench_py_parent", a.bench_parent)):
        if files:
            out[key] = [_bench_line(f) for f in files]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def _child(a, tree):
    """the plain step of ``tree`` in a fresh process (its own library, its own HIP runtime state)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--plain-only", "--runs", str(a.runs), "--window", str(a.window)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child on {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    for ln in reversed(r.stdout.splitlines()):
        if ln.startswith("RESULT "):
            return json.loads(ln[len("RESULT "):])
    raise SystemExit(f"child on {tree} printed no result")


def _bench_line(path):
    """the headline of bench.py's one JSON result line"""
    for ln in reversed(open(path).read().splitlines()):
        if ln.startswith("{"):
            r = json.loads(ln)
            keep = ("metric", "value", "unit", "images_per_sec", "step_ms", "ms_per_step", "mode")
            return {k: r[k] for k in keep if k in r} or r
    raise SystemExit(f"{path} holds no JSON result line")


def alone(torch, fn, n=200):
    """us per call: n back-to-back calls between two device events, after 10 to warm up"""
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


def measure(a, plain_only):
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import _lib, ops
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion import ddpm as D
    assert torch.cuda.is_available(), "distill_bench needs a GPU: it does not fall back"
    assert os.path.abspath(_lib.LIB_PATH).startswith(root), f"library {_lib.LIB_PATH} is not the one of {root}"
    dev = torch.device("cuda", 0)

    def module(size, **kw):
        torch.manual_seed(0)
        m = D.DDPM(img_channels=3, img_size=size, dim=64, lr=8e-5, **kw)
        m.sample_every = 0
        m.to(dev)
        m.prepare_hip(dev)
        m.train()
        return m, m.configure_optimizers()

    g = torch.Generator().manual_seed(1)

    def fast_steps(fast, x):
        def run(n):
            for i in range(n):
                fast.step((x, None), i)
        return run

    def timed(variants):
        for run in variants.values():
            run(3)
        wall = {k: [] for k in variants}
        for _ in range(a.runs):
            for k, run in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.window)
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3 / a.window)
        return {k: round(statistics.median(v), 4) for k, v in wall.items()}, {k: [round(t, 3) for t in v] for k, v in wall.items()}

    B, S, C = 128, 32, 3
    x = torch.rand(B, C, S, S, generator=g).to(dev)
    if plain_only:
        fast = DDPMFastStep(*module(S), 1, use_graph=True)
        ms, windows = timed({"plain": fast_steps(fast, x)})
        assert fast.mode.startswith("hipGraph")
        return {"tree": root, "plain_step_ms": ms["plain"], "windows_ms": windows["plain"]}

    out = {"what": f"UNet dim 64, one GPU, graph replay; ms per step: wall time of windows of {a.window} steps "
                   f"(torch.cuda.synchronize on both sides), median of {a.runs} windows after warm-up, the variants of one process "
                   f"alternating; us figures: 200 back-to-back calls between two device events",
           "device": torch.cuda.get_device_name(0)}
    # ---- (ii) the step at 32 x 32, B = 128
    steps = {"plain": DDPMFastStep(*module(S), 1, use_graph=True),
             "distilling N=128": DDPMFastStep(*module(S, distill_steps=128), 1, use_graph=True)}
    ms, windows = timed({k: fast_steps(f, x) for k, f in steps.items()})
    for k, f in steps.items():
        assert f.mode.startswith("hipGraph"), f"{k}: graph replay is unavailable, the figures would be eager launches"
    out["step_32_B128_ms"], out["step_32_B128_windows_ms"] = ms, windows
    out["step_32_B128_distillation_added_ms"] = round(ms["distilling N=128"] - ms["plain"], 4)
    gd = steps["distilling N=128"].model.ema.online_model
    d, net = gd._distill, gd.model
    del steps

    # ---- (iii) the pieces alone: two teacher forwards (eager launches, no saved activations), the two kernels, q_sample
    noise = torch.randn(B, C, S, S, generator=g).to(dev)
    t = d.levels[torch.randint(0, d.steps, (B,), generator=g).to(dev)]
    q = D.hip_loss_qsample(gd, x, t, noise, True)
    tnet = d.teacher
    out1, _ = tnet.forward_nhwc(q.xt, t, False, True, None)
    xmid, t_mid = tnet.input_buffer(B, S, S, q.xt), torch.empty_like(t)
    to, so = D.OBJECTIVES[d.objective], D.OBJECTIVES[gd.objective]
    half = lambda: ops.distill_half_step(q.xt, 0, out1, t, d.table, to, True, xmid, 0, t_mid, C)                  # noqa: E731
    targ = lambda: ops.distill_target(q.xt, 0, xmid, 0, out1, t, d.table, to, so, True, q.target, C)             # noqa: E731
    L, st = ops.lib(), ops.stream()

    def qsample():
        L.lgm_qsample_target_slice(x.data_ptr(), noise.data_ptr(), None, 0.0, t.data_ptr(), gd.sqrt_alphas_cumprod.data_ptr(),
                                   gd.sqrt_one_minus_alphas_cumprod.data_ptr(), 1, so, q.xt.data_ptr(), net.in_pitch, net.x_off, -1,
                                   q.target.data_ptr(), 4, B, C, S * S, 4, st)
    px = B * S * S * 4 * 4                                                     # bytes of one [B, S, S, 4] buffer
    bytes_ = {"qsample_target_slice": 2 * 4 * B * C * S * S + 2 * px, "distill_half_step": 3 * px, "distill_target": 4 * px}
    us = {"qsample_target_slice": alone(torch, qsample), "distill_half_step": alone(torch, half), "distill_target": alone(torch, targ)}
    fwd_us = alone(torch, lambda: tnet.forward_nhwc(q.xt, t, False, False, None), n=30)
    out["pieces_alone_B128_3x32x32"] = {
        "us": us, "algorithmic_bytes": bytes_, "TB_per_s": {k: round(bytes_[k] / us[k] * 1e-6, 3) for k in us},
        "teacher_forward_without_saved_activations_us (eager launches, host-bound where the host is slower)": fwd_us,
        "two_forwards_and_two_kernels_us": round(2 * fwd_us + us["distill_half_step"] + us["distill_target"], 1)}

    # ---- (iv) one sampled batch of 64 at 64 x 64: time only
    Bs = 64
    nets = D.Unet(dim=64)
    chains = {"ddim 4 (distilled student)": dict(sampling_timesteps=4), "ddim 8 (distilled student)": dict(sampling_timesteps=8),
              "ddim 250": dict(sampling_timesteps=250), "dpm++ 20": dict(sampling_timesteps=20, sampler="dpm++")}
    gds = {k: D.GaussianDiffusion(nets, img_size=64, **kw).to(dev) for k, kw in chains.items()}
    nets.prepare_hip(dev)
    res = {}
    with torch.no_grad():
        for k, gd_ in gds.items():
            gd_.sample(batch_size=Bs)                                          # capture, plans
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gd_.sample(batch_size=Bs)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            res[k] = round(statistics.median(ts), 2)
    out["sample_64_at_64x64_ms (time only: untrained networks, sample quality at these step counts is not measured)"] = res
    return out


if __name__ == "__main__":
    main()
