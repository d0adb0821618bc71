"""Time low-resolution conditioning (``DDPM(lowres_cond=True)``, a super-resolution stage) on one GPU.

Random weights and data, graph replay.  Step figures are the median over ``--runs`` windows (``torch.cuda.synchronize`` on both
sides of a window of ``--window`` steps) after warm-up, the variants of one process alternating window by window, as
tools/dropout_bench.py does:

  (i)   the plain 32 x 32 step (UNet dim 64, B = 128) on this tree and, with ``--parent-tree DIR``, on another checkout (the
        parent commit with its own library): fresh child processes started from this call, alternating tree by tree,
        ``--rounds`` each - the update launchers gained an extent, a plain model must not have moved;
  (ii)  the training step at 128 x 128, B = 32, with and without conditioning (factor 4), one process, and the library calls
        of one eager step of each by entry point;
  (iii) between device events, back-to-back launches at [32, 3, 128, 128]: ``lgm_lowres_cond`` (training source, r = 4) beside
        ``lgm_qsample_target_slice`` - the same class of bytes: image and noise in, one slice out - with the bytes each moves,
        the achieved TB/s, their ratio and what the tile halo predicts; the sampling source and r = 2 / 8 beside them;
  (iv)  the time-embedding forward of a conditioned and a plain network (eager launches, B = 32): the five launches the
        augmentation-level embedding adds;
  (v)   one replayed ancestral sampling step at 128 x 128, B = 16, with and without conditioning;
  (vi)  ``--bench FILE ...`` / ``--bench-parent FILE ...``: bench.py's result lines on both trees, copied in.

Usage:  python tools/lowres_bench.py [--parent-tree DIR] [--out profiles/r18_lowres_bench.json] [--bench FILE ...]
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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r18_lowres_bench.json"))
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
    assert torch.cuda.is_available(), "lowres_bench needs a GPU: it does not fall back"
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

    if plain_only:
        x = torch.rand(128, 3, 32, 32, generator=g).to(dev)
        fast = DDPMFastStep(*module(32), 1, use_graph=True)
        ms, windows = timed({"plain": fast_steps(fast, x)})
        assert fast.mode.startswith("hipGraph")
        return {"tree": root, "plain_step_ms": ms["plain"], "windows_ms": windows["plain"]}

    out = {"what": f"UNet dim 64, one GPU, graph replay; ms per step: wall time of windows of {a.window} steps "
                   f"(torch.cuda.synchronize on both sides), median of {a.runs} windows after warm-up, the variants of one process "
                   f"alternating; us figures: 200 back-to-back calls between two device events",
           "device": torch.cuda.get_device_name(0)}
    # ---- (ii) the step at 128 x 128, B = 32
    B = 32
    x128 = torch.rand(B, 3, 128, 128, generator=g).to(dev)
    steps = {"plain": DDPMFastStep(*module(128), 1, use_graph=True),
             "lowres_cond": DDPMFastStep(*module(128, lowres_cond=True), 1, use_graph=True)}
    ms, windows = timed({k: fast_steps(f, x128) for k, f in steps.items()})
    for k, f in steps.items():
        assert f.mode.startswith("hipGraph"), f"{k}: graph replay is unavailable, the figures would be eager launches"
    out["step_128_B32_ms"], out["step_128_B32_windows_ms"] = ms, windows
    out["step_128_B32_conditioning_added_us"] = round((ms["lowres_cond"] - ms["plain"]) * 1e3, 1)

    def calls_of(**kw):
        m, opt = module(128, **kw)
        fast = DDPMFastStep(m, opt, 1, use_graph=False)
        fast.step((x128, None), 0)                          # allocations, plans
        L = ops.lib()
        seen, saved = {}, {}
        for name in L.protos:
            fn = getattr(L, name)
            saved[name] = fn

            def wrap(*args, _fn=fn, _n=name):
                seen[_n] = seen.get(_n, 0) + 1
                return _fn(*args)
            setattr(L, name, wrap)
        try:
            fast.step((x128, None), 1)
        finally:
            for name, fn in saved.items():
                setattr(L, name, fn)
        torch.cuda.synchronize()
        return seen
    pc, cc = calls_of(), calls_of(lowres_cond=True)
    out["library_calls_one_eager_step: entry points whose count differs [plain, lowres_cond]"] = {
        k: [pc.get(k, 0), cc.get(k, 0)] for k in sorted(set(pc) | set(cc)) if pc.get(k, 0) != cc.get(k, 0)}
    del steps

    # ---- (iii) the producer of the slice alone, beside q_sample's
    gd = D.GaussianDiffusion(D.Unet(dim=64, lowres_cond=True), img_size=128).to(dev)
    net = gd.model
    C, S = 3, 128
    img, noise = x128, torch.randn(B, C, S, S, generator=g).to(dev)
    s = torch.randint(0, 1000, (B,), generator=g).to(dev)
    xin = torch.zeros(B, S, S, net.in_pitch, device=dev)
    target = torch.zeros(B, S, S, 4, device=dev)
    L, st = ops.lib(), ops.stream()
    tabs = dict(sqrt_ac=gd.sqrt_alphas_cumprod, sqrt_1mac=gd.sqrt_one_minus_alphas_cumprod)

    def qsample():
        L.lgm_qsample_target_slice(img.data_ptr(), noise.data_ptr(), None, 0.0, s.data_ptr(), tabs["sqrt_ac"].data_ptr(),
                                   tabs["sqrt_1mac"].data_ptr(), 1, 2, xin.data_ptr(), net.in_pitch, net.x_off, -1,
                                   target.data_ptr(), 4, B, C, S * S, 4, st)
    n_el = B * C * S * S
    q_bytes = 4 * (2 * n_el + B * S * S * net.in_pitch + B * S * S * 4)            # img + noise in; the whole pitch + target out
    k_us = {}
    k_us["qsample_target_slice"] = alone(torch, qsample)
    k_us["lowres_cond img r=4"] = alone(torch, lambda: ops.lowres_cond(xin, 0, C, 4, img=img, eps=noise, s=s, normalize=True, **tabs))
    for r in (2, 8):
        k_us[f"lowres_cond img r={r}"] = alone(torch, lambda: ops.lowres_cond(xin, 0, C, r, img=img, eps=noise, s=s, normalize=True, **tabs))
    low = torch.rand(B, C, S // 4, S // 4, generator=g).to(dev)
    k_us["lowres_cond low r=4"] = alone(torch, lambda: ops.lowres_cond(xin, 0, C, 4, low=low, eps=noise, s=s, normalize=True, **tabs))
    k_us["lowres_cond img r=4, eps NULL"] = alone(torch, lambda: ops.lowres_cond(xin, 0, C, 4, img=img, normalize=True))
    l_bytes = 4 * (2 * n_el + n_el)                                                   # img + eps in; one slice out
    out["kernels_alone_B32_3x128x128"] = {
        "us": k_us,
        "algorithmic_bytes": {"qsample_target_slice": q_bytes, "lowres_cond img": l_bytes},
        "TB_per_s": {"qsample_target_slice": round(q_bytes / k_us["qsample_target_slice"] * 1e-6, 3),
                     "lowres_cond img r=4": round(l_bytes / k_us["lowres_cond img r=4"] * 1e-6, 3)},
        "lowres_over_qsample_time": round(k_us["lowres_cond img r=4"] / k_us["qsample_target_slice"], 3),
        "lowres_over_qsample_bytes": round(l_bytes / q_bytes, 3),
        "halo": "a workgroup reads (8 + 2)(16 + 2) low-resolution pixels' blocks for 8 x 16 of its own: at most 1.41 x the image, "
                "served from L2 where a neighbour has read it; 32 x 32 low-resolution maps are 4 x 2 tiles per sample"}

    # ---- (iv) the time-embedding forward, conditioned and plain (eager launches)
    plain_net = D.Unet(dim=64)
    D.GaussianDiffusion(plain_net, img_size=128).to(dev)
    plain_net.prepare_hip(dev)
    net.prepare_hip(dev)
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    emb = {"plain": alone(torch, lambda: plain_net._time_fwd(t, False)),
           "lowres_cond": alone(torch, lambda: net._time_fwd(t, False, None, s))}
    emb["added_us (5 launches: posemb, linear, GELU, linear, add + SiLU; the SiLU launch it replaces is gone)"] = round(
        emb["lowres_cond"] - emb["plain"], 3)
    out["time_embedding_forward_eager_us"] = emb

    # ---- (v) one replayed ancestral sampling step at 128 x 128, B = 16
    from lgm_hip import sampler
    Bs, n = 16, 40
    shape = (Bs, 3, 128, 128)
    gdp = D.GaussianDiffusion(plain_net, img_size=128).to(dev)
    low16 = torch.rand(Bs, 3, 32, 32, generator=g).to(dev)

    def chain(gd_, lr):
        def run(k):
            for _ in range(k):
                sampler._run(gd_, shape, sampler._plan_ancestral(gd_, steps=n), lowres=lr)
        return run
    with torch.no_grad():
        ms, windows = timed({"plain": chain(gdp, None), "lowres_cond": chain(gd, dict(lowres=low16))})
    out["sampling_step_128_B16_ms"] = {k: round(v / n, 4) for k, v in ms.items()}
    out["sampling_step_128_B16: chains of"] = n
    return out


if __name__ == "__main__":
    main()
