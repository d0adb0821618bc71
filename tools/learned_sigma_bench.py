"""Time the learned-variance DDPM beside the plain one, one GPU.

DDPM 32 x 32 (UNet dim 64, random weights and data).  Step figures are the median over ``--runs`` windows
(``torch.cuda.synchronize`` on both sides of a window of ``--window`` steps) after warm-up, the variants of one comparison
alternating window by window inside one process, as tools/gradtail_bench.py does:

  (i)   the plain B = 128 training step (``DDPMFastStep``, graph replay) - with ``--tree DIR --parent-only`` the same on another
        checkout (the parent commit with its own library), whose result file ``--parent FILE ...`` puts beside this commit's:
        the default path must not have moved;
  (ii)  the learned-variance step beside it (final_conv 64 -> 6 on the Nw = 8 narrow kernels, the hybrid loss);
  (iii) between device events, back-to-back launches: the hybrid loss forward and backward beside the weighted MSE's, the narrow
        1x1 kernels at Nw = 8 beside Nw = 4 at B = 128, and - ``--fallback-only``, a child process with ``LGM_NO_NARROW1X1=1``,
        taken once - the kernels the 64 -> 6 layer would fall back to;
  (iv)  one graph-replayed ancestral sampling step (B = 64) with the learned variance beside the fixed one;
  (v)   the hybrid loss at 256 x 256, B = 8: one workgroup per sample, eight workgroups in all.

Usage:  python tools/learned_sigma_bench.py [--out profiles/r15_learned_sigma_bench.json] [--parent FILE ...]
        python tools/learned_sigma_bench.py --tree DIR --parent-only --out FILE
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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r15_learned_sigma_bench.json"))
    ap.add_argument("--parent", default=None, nargs="*", help="result files of --parent-only runs on the parent commit")
    ap.add_argument("--parent-only", action="store_true", help="only what another checkout can run: (i)")
    ap.add_argument("--fallback-only", action="store_true", help="(iii)'s fallback figures alone, printed as JSON (child process)")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    a = ap.parse_args()
    if a.fallback_only:
        print(json.dumps(narrow_alone(a, here, (8,))))
        return
    out = measure(a, here)
    if a.parent:
        bases = [json.load(open(f)) for f in a.parent]
        out["parent_commit"] = [{"plain_step_ms": b["plain_step_ms"]} for b in bases]
        out["plain_step_over_parent"] = round(out["plain_step_ms"] / statistics.median(b["plain_step_ms"] for b in bases), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def _paths(a):
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    return root


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


def narrow_alone(a, here, widths):
    """{name: us} of the 1x1 layer 64 -> Nw and its input gradient at B = 128, 32 x 32, and the kernels that ran"""
    _paths(a)
    import torch
    from lgm_hip import ops
    dev = torch.device("cuda", 0)
    out = {}
    P = 128 * 32 * 32
    x = torch.randn(128, 32, 32, 64, device=dev)
    for nw in widths:
        g = ops.make_geom(128, 32, 32, 64, nw, 1, 1, 1, 0)
        w, b = torch.randn(nw, 1, 64, device=dev), torch.randn(nw, device=dev)
        wt = w.permute(2, 1, 0).contiguous()
        y, gx = torch.empty(128, 32, 32, nw, device=dev), torch.empty_like(x)
        out[f"fwd_nw{nw}_us"] = alone(torch, lambda: ops.conv_xy(g, x, w.data_ptr(), b.data_ptr(), None, y))
        out[f"fwd_nw{nw}_kernel"] = ops.lib()._dll.lgm_last_kernel().decode()
        out[f"dgrad_nw{nw}_us"] = alone(torch, lambda: ops.conv_yx(g, y, w.data_ptr(), None, None, gx, wt.data_ptr()))
        out[f"dgrad_nw{nw}_kernel"] = ops.lib()._dll.lgm_last_kernel().decode()
        out[f"fwd_nw{nw}_GBps"] = round((P * 64 + P * nw) * 4 / out[f"fwd_nw{nw}_us"] * 1e-3, 1)
    return out


def measure(a, here):
    root = _paths(a)
    import torch
    from lgm_hip import ops
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion import ddpm as D
    assert torch.cuda.is_available(), "learned_sigma_bench needs a GPU: it does not fall back"
    dev = torch.device("cuda", 0)
    FULL = 128

    def module(**kw):
        torch.manual_seed(0)
        m = D.DDPM(img_channels=3, img_size=32, dim=64, lr=8e-5, **kw)
        m.sample_every = 0
        m.to(dev)
        m.prepare_hip(dev)
        m.train()
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

    out = {"what": f"DDPM 32 x 32, UNet dim 64, one GPU; ms per step: wall time of windows of {a.window} steps "
                   f"(torch.cuda.synchronize on both sides), median of {a.runs} windows after warm-up, the variants of one "
                   f"comparison alternating; us figures: 200 back-to-back launches between two device events",
           "device": torch.cuda.get_device_name(0), "tree": "this commit" if root == here else "parent commit"}
    m0, o0 = module()
    plain = DDPMFastStep(m0, o0, 1, use_graph=True)
    variants = {"plain": fast_steps(plain)}
    if not a.parent_only:
        m1, o1 = module(learned_variance=True)
        learned = DDPMFastStep(m1, o1, 1, use_graph=True)
        variants["learned"] = fast_steps(learned)
    ms, windows = timed(variants)
    assert plain.mode.startswith("hipGraph"), "graph replay is unavailable: the figures would be eager launches"
    out["plain_step_ms"], out["windows_ms"] = ms["plain"], windows
    if a.parent_only:
        return out
    assert learned.mode.startswith("hipGraph")
    out["learned_step_ms"] = ms["learned"]
    out["learned_step_added_us"] = round((ms["learned"] - ms["plain"]) * 1e3, 1)

    # (iii) the loss launches alone, at the step's shapes and at 256 x 256
    def loss_alone(B, S):
        gd_l, gd_p = m1.ema.online_model, m0.ema.online_model
        gg = torch.Generator().manual_seed(2)
        img = torch.rand(B, 3, S, S, generator=gg).to(dev)
        nz = torch.randn(B, 3, S, S, generator=gg).to(dev)
        t = torch.randint(0, 1000, (B,), generator=gg).to(dev)
        t[0] = 0
        q = D.hip_loss_qsample(gd_l, img, t, nz, True)
        target, t = q.target, q.t
        out8 = torch.randn(B, S, S, 8, device=dev)
        out4 = out8[..., :4].contiguous()
        per2, per1, loss = torch.empty(2, B, device=dev), torch.empty(B, device=dev), torch.empty(1, device=dev)
        g8, g4, one = torch.empty_like(out8), torch.empty_like(out4), torch.ones(1, device=dev)
        L, st = ops.lib(), ops.stream()
        ctx = D.LossContext(gd_l, None, out8, target, t, tuple(q.img.shape), q.img, q.noise, q.offset)
        ctx.xt, ctx.normalize = q.xt, True
        head = D._loss_form(ctx)[1]
        lw = gd_p.loss_weight.data_ptr()
        return {
            "hybrid_fwd_us": alone(torch, lambda: L.lgm_hybrid_loss_fwd(*head, B, 3, S * S, per2.data_ptr(), loss.data_ptr(), st)),
            "hybrid_bwd_us": alone(torch, lambda: L.lgm_hybrid_loss_bwd(*head, one.data_ptr(), B, 3, S * S, g8.data_ptr(), st)),
            "weighted_mse_fwd_us": alone(torch, lambda: L.lgm_weighted_mse_fwd(out4.data_ptr(), target.data_ptr(), 4, t.data_ptr(), lw,
                                                                              B, 3, S * S, 4, per1.data_ptr(), loss.data_ptr(), st)),
            "weighted_mse_bwd_us": alone(torch, lambda: L.lgm_weighted_mse_bwd(out4.data_ptr(), target.data_ptr(), 4, t.data_ptr(), lw,
                                                                              one.data_ptr(), B, 3, S * S, 4, g4.data_ptr(), st))}
    out["loss_alone_B128_32x32"] = loss_alone(FULL, 32)
    out["loss_alone_B8_256x256"] = loss_alone(8, 256)
    out["narrow1x1_alone_B128_32x32"] = narrow_alone(a, here, (4, 8))
    env = dict(os.environ, LGM_NO_NARROW1X1="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--fallback-only"], env=env, check=True,
                           capture_output=True, text=True)
    out["narrow1x1_fallback_B128_32x32"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps({k: out[k] for k in out if k.startswith(("loss_alone", "narrow1x1"))}), flush=True)

    # (iv) one graph-replayed ancestral step, learned beside fixed
    from lgm_hip import sampler
    shape = (64, 3, 32, 32)
    gds = {"fixed": m0.ema.ema_model, "learned": m1.ema.ema_model}
    for gd in gds.values():
        gd.eval()
        assert sampler.warm_chain(gd, shape), "graph replay is unavailable"
    steps = 20

    def chain(gd):
        plan = sampler._plan_ancestral(gd, steps=steps)
        return lambda n: [sampler._run(gd, shape, plan) for _ in range(n)]
    with torch.no_grad():
        ms, windows = timed({k: chain(gd) for k, gd in gds.items()})
    out["ancestral_step_ms"] = {k: round(v / steps, 4) for k, v in ms.items()}
    out["ancestral_step_learned_added_us"] = round((ms["learned"] - ms["fixed"]) / steps * 1e3, 1)
    return out


if __name__ == "__main__":
    main()
