"""Time the timestep samplers of the DDPM training step (``t_sampler=...``) beside the uniform draw, one GPU.

DDPM 32 x 32 (UNet dim 64, random weights and data), B = 128, graph replay.  Step figures are the median over ``--runs`` windows
(``torch.cuda.synchronize`` on both sides of a window of ``--window`` steps) after warm-up, the variants of one comparison
alternating window by window inside one process, as tools/learned_sigma_bench.py does:

  (i)   the ``"uniform"`` step - with ``--tree DIR --parent-only`` the same on another checkout (the parent commit with its own
        library), whose result file ``--parent FILE ...`` puts beside this commit's: the default path must not have moved;
  (ii)  the ``"stratified"`` and the ``"loss_second_moment"`` step beside it (the latter pre-loaded to warm, so that the weighted
        loss kernels and a non-uniform plan are what is timed), plain and learned-variance network;
  (iii) between device events, back-to-back launches at T = 1000: lgm_tsampler_draw (both modes) and lgm_tsampler_update for
        B = 128 and B = 16, the update of a batch that repeats one timestep, and - in the same process - the hybrid loss
        forward the update kernel is to be compared with;
  (iv)  ``--bench FILE ...`` / ``--bench-parent FILE ...``: bench.py's result lines on both trees, copied in.

Usage:  python tools/tsampler_bench.py [--out profiles/r16_tsampler_bench.json] [--parent FILE ...] [--bench FILE ...]
        python tools/tsampler_bench.py --tree DIR --parent-only --out FILE
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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r16_tsampler_bench.json"))
    ap.add_argument("--parent", default=None, nargs="*", help="result files of --parent-only runs on the parent commit")
    ap.add_argument("--parent-only", action="store_true", help="only what another checkout can run: (i)")
    ap.add_argument("--bench", default=None, nargs="*", help="files holding bench.py's JSON result line, this commit")
    ap.add_argument("--bench-parent", default=None, nargs="*", help="the same from the parent commit's tree")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    a = ap.parse_args()
    out = measure(a, here)
    if a.parent:
        bases = [json.load(open(f)) for f in a.parent]
        out["parent_commit"] = [{"uniform_step_ms": b["uniform_step_ms"]} for b in bases]
        out["uniform_step_over_parent"] = round(out["uniform_step_ms"] / statistics.median(b["uniform_step_ms"] for b in bases), 4)
    for key, files in (("bench_py", a.bench), ("bench_py_parent", a.bench_parent)):
        if files:
            out[key] = [_bench_line(f) for f in files]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def _bench_line(path):
    """the headline of bench.py's one JSON result line"""
    for ln in reversed(open(path).read().splitlines()):
        if ln.startswith("{"):
            r = json.loads(ln)
            keep = ("metric", "value", "unit", "images_per_sec", "step_ms", "ms_per_step", "mode")
            return {k: r[k] for k in keep if k in r} or r
    raise SystemExit(f"{path} holds no JSON result line")


def alone(torch, fn, n=200):
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


def measure(a, here):
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion import ddpm as D
    assert torch.cuda.is_available(), "tsampler_bench needs a GPU: it does not fall back"
    dev = torch.device("cuda", 0)
    FULL, T, H = 128, 1000, 10

    def warm_history(seed=0):
        g = torch.Generator().manual_seed(seed)
        scale = 10.0 ** (-3.0 * torch.rand(T, 1, generator=g))
        return (scale * (0.5 + torch.randn(T, H, generator=g).abs())).to(dev), torch.full((T,), H, dtype=torch.int32, device=dev)

    def module(**kw):
        torch.manual_seed(0)
        m = D.DDPM(img_channels=3, img_size=32, dim=64, lr=8e-5, **kw)
        m.sample_every = 0
        m.to(dev)
        m.prepare_hip(dev)
        m.train()
        if kw.get("t_sampler") == "loss_second_moment":
            m.ema.online_model._ts.load_state(*warm_history())
        return m, m.configure_optimizers()

    g = torch.Generator().manual_seed(1)
    x_full = torch.rand(FULL, 3, 32, 32, generator=g).to(dev)

    def fast_steps(fast):
        def run(n):
            for i in range(n):
                fast.step((x_full, None), i)
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

    out = {"what": f"DDPM 32 x 32, UNet dim 64, B = {FULL}, one GPU, graph replay; ms per step: wall time of windows of "
                   f"{a.window} steps (torch.cuda.synchronize on both sides), median of {a.runs} windows after warm-up, the "
                   f"variants of one comparison alternating; us figures: 200 back-to-back launches between two device events",
           "device": torch.cuda.get_device_name(0), "tree": "this commit" if root == here else "parent commit"}
    steps = {}
    m0, o0 = module()
    steps["uniform"] = DDPMFastStep(m0, o0, 1, use_graph=True)
    if not a.parent_only:
        for name, kw in (("stratified", dict(t_sampler="stratified")), ("loss_second_moment", dict(t_sampler="loss_second_moment")),
                         ("learned_uniform", dict(learned_variance=True)),
                         ("learned_loss_second_moment", dict(learned_variance=True, t_sampler="loss_second_moment"))):
            steps[name] = DDPMFastStep(*module(**kw), 1, use_graph=True)
    ms, windows = timed({k: fast_steps(f) for k, f in steps.items()})
    for k, f in steps.items():
        assert f.mode.startswith("hipGraph"), f"{k}: graph replay is unavailable, the figures would be eager launches"
    out["uniform_step_ms"], out["windows_ms"] = ms["uniform"], windows
    if a.parent_only:
        return out
    out["step_ms"] = ms
    out["added_us"] = {"stratified": round((ms["stratified"] - ms["uniform"]) * 1e3, 1),
                       "loss_second_moment": round((ms["loss_second_moment"] - ms["uniform"]) * 1e3, 1),
                       "learned_loss_second_moment": round((ms["learned_loss_second_moment"] - ms["learned_uniform"]) * 1e3, 1)}
    ts = steps["loss_second_moment"].model.ema.online_model._ts
    out["loss_second_moment_rows_full_after_run"] = ts.warm_fraction()

    # (iii) the launches alone
    L, st = ops.lib(), ops.stream()
    hist, counts = warm_history(1)
    cdf, iw = torch.empty(T, device=dev), torch.empty(T, device=dev)
    L.lgm_tsampler_update(None, None, 1, 0.0, hist.data_ptr(), counts.data_ptr(), H, 0.001, T, 0, cdf.data_ptr(), iw.data_ptr(), st)
    launches = {}
    for B in (128, 16):
        gg = torch.Generator().manual_seed(B)
        u = torch.rand(B, generator=gg).to(dev)
        t = torch.randint(0, T, (B,), generator=gg).to(dev)
        same = torch.full((B,), 7, dtype=torch.long, device=dev)
        per = torch.rand(2, B, generator=gg).to(dev)
        tout = torch.empty(B, dtype=torch.long, device=dev)

        def update(tt, n_terms):
            return lambda: L.lgm_tsampler_update(tt.data_ptr(), per.data_ptr(), n_terms, 0.001, hist.data_ptr(), counts.data_ptr(), H,
                                                 0.001, T, B, cdf.data_ptr(), iw.data_ptr(), st)
        launches[f"B{B}"] = {
            "draw_cdf_us": alone(torch, lambda: L.lgm_tsampler_draw(u.data_ptr(), cdf.data_ptr(), T, 1, tout.data_ptr(), B, st)),
            "draw_stratified_us": alone(torch, lambda: L.lgm_tsampler_draw(u.data_ptr(), None, T, 0, tout.data_ptr(), B, st)),
            "update_us": alone(torch, update(t, 1)),
            "update_two_terms_us": alone(torch, update(t, 2)),
            "update_one_timestep_repeated_us": alone(torch, update(same, 1))}
    launches["plan_only_us"] = alone(torch, lambda: L.lgm_tsampler_update(None, None, 1, 0.0, hist.data_ptr(), counts.data_ptr(), H,
                                                                          0.001, T, 0, cdf.data_ptr(), iw.data_ptr(), st))
    # the hybrid loss forward at the step's shapes, in this process: what the update kernel is compared with
    gd_l = steps["learned_uniform"].model.ema.online_model
    gg = torch.Generator().manual_seed(2)
    img, nz = torch.rand(FULL, 3, 32, 32, generator=gg).to(dev), torch.randn(FULL, 3, 32, 32, generator=gg).to(dev)
    t = torch.randint(0, T, (FULL,), generator=gg).to(dev)
    q = D.hip_loss_qsample(gd_l, img, t, nz, True)
    out8 = torch.randn(FULL, 32, 32, 8, device=dev)
    per2, wb, loss = torch.empty(2, FULL, device=dev), torch.empty(FULL, device=dev), torch.empty(1, device=dev)
    ctx = D.LossContext(gd_l, None, out8, q.target, q.t, tuple(q.img.shape), q.img, q.noise, q.offset)
    ctx.xt, ctx.normalize = q.xt, True
    head = D._loss_form(ctx)[1]
    launches["hybrid_fwd_us"] = alone(torch, lambda: L.lgm_hybrid_loss_fwd(*head, FULL, 3, 32 * 32, per2.data_ptr(), loss.data_ptr(), st))
    launches["hybrid_fwd_iw_us"] = alone(torch, lambda: L.lgm_hybrid_loss_fwd_iw(*head, iw.data_ptr(), FULL, 3, 32 * 32, per2.data_ptr(),
                                                                                 wb.data_ptr(), loss.data_ptr(), st))
    out["launches_alone_T1000"] = launches
    return out


if __name__ == "__main__":
    main()
