"""Measure the MLP VAE on the HIP path -> profiles/r23_vae_bench.json.  Needs a GPU; nothing falls back.

  (i)   every dense kernel on the layer shapes of configs/vae/vae.json at B = 32 and B = 256 beside the generic entry point on the
        SAME operands in the same process (``ops.conv_xy`` with the LeakyReLU post-op / ``ops.conv_bwd_generic`` at
        [B, 1, 1, C]; "bwd" times the generic backward without the activation's derivative, which the dense one has in it,
        "bwd_act" with the elementwise launch in front that supplies it); the heads and the loss kernels alone: median of
        ``--runs`` alternating windows of ``--window`` calls between device events;
  (ii)  the training step at B = 32 (the config) and B = 256: graph replay, the same step object issuing eager launches, and -
        with ``--parent DIR``, a checkout of the parent commit - that tree's step on the same device (eager ATen +
        ``torch.optim.Adam``), and the replayed step under every other (fwd, bwd) route of ``lgm_hip.nn.Linear``, the
        candidates taking turns;
  (iii) with ``--parent DIR`` (its library built): ``bench.py`` (DDPM 32 x 32 and ``--workload vqvae``) on this tree and on the
        parent's, alternating, ``--bench-rounds`` times each.
TIME ONLY: the networks are untrained.

Usage:  python tools/vae_bench.py [--parent DIR] [--bench-rounds N]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys


def window(torch, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def alternate(torch, fns, runs, n):
    """{name: median us per call} over ``runs`` windows of ``n`` calls each, the candidates taking turns"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            got[k].append(window(torch, fn, n))
    return {k: round(statistics.median(v), 2) for k, v in got.items()}


def _bench_line(text):
    for ln in reversed(text.splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("bench.py printed no JSON result line")


def _parent_vae(parent):
    path = os.path.join(parent, "lightning-generative-models_amd", "models", "generative", "vae", "vae.py")
    spec = importlib.util.spec_from_file_location("parent_vae", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VAE


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r23_vae_bench.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (bench.py needs its library built)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=20)
    a = ap.parse_args()
    for p in (here, os.path.join(here, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops
    from utils.loader import load_config, load_model
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    rec = {"runs": a.runs, "window": a.window, "unit": "us per call, median of alternating windows", "kernels": {}}
    cfg = load_config(os.path.join(here, "lightning-generative-models_amd", "configs", "vae", "vae.json"))

    # (i) kernels
    r4 = lambda n: (n + 3) // 4 * 4                                   # noqa: E731
    layers = [(784, 512), (512, 256), (256, 128), (20, 128), (128, 256), (256, 512), (512, 784)]
    for B in (32, 256):
        for K, N in layers:
            gen = torch.Generator().manual_seed(K + N)
            Kp, Np = r4(K), r4(N)
            x = torch.randn(B, Kp, generator=gen).to(dev)
            w = (torch.randn(Np, Kp, generator=gen) / K ** 0.5).to(dev)
            wt = w.t().contiguous()
            bias, gy = torch.randn(Np, generator=gen).to(dev), torch.randn(B, Np, generator=gen).to(dev)
            y, y2 = torch.empty(B, Np, device=dev), torch.empty(B, Np, device=dev)
            gx, gx2 = torch.empty(B, Kp, device=dev), torch.empty(B, Kp, device=dev)
            gw, gb, gw2, gb2 = torch.empty_like(w), torch.empty_like(bias), torch.empty_like(w), torch.empty_like(bias)
            g = ops.make_geom(B, 1, 1, Kp, Np, 1, 1, 1, 0)
            x4, y4, gy4, gx4 = x.view(B, 1, 1, Kp), y2.view(B, 1, 1, Np), gy.view(B, 1, 1, Np), gx2.view(B, 1, 1, Kp)
            post = ops.make_post(ops.ACT_LRELU, 0.2)
            y4d, g4 = y.view(B, 1, 1, Np), torch.empty(B, 1, 1, Np, device=dev)
            ops.dense_fwd(x, w.data_ptr(), bias.data_ptr(), K, N, y, ops.ACT_LRELU, 0.2)
            cases = {
                "fwd": {"dense": lambda: ops.dense_fwd(x, w.data_ptr(), bias.data_ptr(), K, N, y, ops.ACT_LRELU, 0.2),
                        "generic": lambda: ops.conv_xy(g, x4, w.data_ptr(), bias.data_ptr(), None, y4, post=post)},
                "bwd": {"dense": lambda: ops.dense_bwd(gy, y, x, wt.data_ptr(), K, N, gx, gw.data_ptr(), gb.data_ptr(), 0.0,
                                                       ops.ACT_LRELU, 0.2),
                        "generic": lambda: ops.conv_bwd_generic(g, gy4, x4, w.data_ptr(), wt.data_ptr(), gw2.data_ptr(), 0.0,
                                                                gb2.data_ptr(), None, None, gx4)},
                "bwd_act": {"dense": lambda: ops.dense_bwd(gy, y, x, wt.data_ptr(), K, N, gx, gw.data_ptr(), gb.data_ptr(), 0.0,
                                                           ops.ACT_LRELU, 0.2),
                            "generic": lambda: (ops.act_bwd(y4d, None, gy4, g4, False, ops.ACT_LRELU, 0.2),
                                                ops.conv_bwd_generic(g, g4, x4, w.data_ptr(), wt.data_ptr(), gw2.data_ptr(), 0.0,
                                                                     gb2.data_ptr(), None, None, gx4))},
                "bwd_no_gx": {"dense": lambda: ops.dense_bwd(gy, y, x, None, K, N, None, gw.data_ptr(), gb.data_ptr(), 0.0,
                                                             ops.ACT_LRELU, 0.2),
                              "generic": lambda: ops.conv_wgrad(g, gy4, x4, gw2.data_ptr(), 0.0, gb2.data_ptr())},
            }
            for name, fns in cases.items():
                t = alternate(torch, fns, a.runs, a.window)
                t["dense_over_generic"] = round(t["dense"] / t["generic"], 3)
                rec["kernels"][f"{name} B{B} {K}->{N}"] = t
                print(f"{name} B{B} {K}->{N}: {t}", flush=True)
            rec["kernels"][f"fwd B{B} {K}->{N}"]["rel_diff_dense_vs_generic"] = float((y - y2).norm() / y2.norm())
        # heads and loss, alone
        L, D = 20, 784
        gen = torch.Generator().manual_seed(B)
        h, eps = torch.randn(B, 128, generator=gen).to(dev), torch.randn(B, L, generator=gen).to(dev)
        W = [(torch.randn(L, 128, generator=gen) * 0.05).to(dev) for _ in range(2)]
        bs = [torch.zeros(L, device=dev) for _ in range(2)]
        mu, lv, z, part = ops.vae_head_fwd(h, 128, L, W[0].data_ptr(), bs[0].data_ptr(), W[1].data_ptr(), bs[1].data_ptr(), eps)
        gz, gl = torch.randn(B, L, generator=gen).to(dev), torch.ones(1, device=dev)
        gh = torch.empty(B, 128, device=dev)
        GW, GB = [torch.empty_like(v) for v in W], [torch.empty_like(v) for v in bs]
        pre, img = torch.randn(B, D, generator=gen).to(dev), torch.rand(B, D, generator=gen).to(dev)
        xh, row, gpre, vals = torch.empty(B, D, device=dev), torch.empty(B, device=dev), torch.empty(B, D, device=dev), \
            torch.empty(3, device=dev)
        t = alternate(torch, {
            "vae_head_fwd": lambda: ops.vae_head_fwd(h, 128, L, W[0].data_ptr(), bs[0].data_ptr(), W[1].data_ptr(),
                                                     bs[1].data_ptr(), eps),
            "vae_head_bwd": lambda: ops.vae_head_bwd(gz, mu, lv, eps, gl, 0.01, h, 128, L, W[0].data_ptr(), W[1].data_ptr(), gh,
                                                     GW[0].data_ptr(), GB[0].data_ptr(), GW[1].data_ptr(), GB[1].data_ptr(), 0.0),
            "tanh_l1_fwd": lambda: ops.tanh_l1_fwd(pre, img, D, xh, row),
            "tanh_l1_bwd": lambda: ops.tanh_l1_bwd(xh, img, gl, D, gpre),
            "vae_loss": lambda: ops.vae_loss(row, part, D, L, 0.01, vals)}, a.runs, a.window)
        rec["kernels"][f"heads and loss B{B}"] = t
        print(f"heads and loss B{B}: {t}", flush=True)

    # (ii) the training step
    rec["train_step"] = {}
    for B in (32, 256):
        img = torch.rand(B, 1, 28, 28, device=dev) * 2 - 1
        batch = (img, None)
        fns, keep = {}, []
        from lgm_hip.nn import Linear
        default_routes = (Linear.fwd_route, Linear.bwd_route)
        variants = [("replay", True, default_routes), ("eager_launches", False, default_routes)]
        variants += [(f"replay fwd={f} bwd={b_}", True, (f, b_)) for f in ("dense", "generic") for b_ in ("dense", "generic")
                     if (f, b_) != default_routes]
        for name, graph, routes in variants:             # a model and a captured step per variant: the routes are baked in
            Linear.fwd_route, Linear.bwd_route = routes
            torch.manual_seed(0)
            m = load_model(cfg["model"]).to(dev)
            m.prepare_hip(dev)
            m.train()
            fast = m.make_fast_step(m.configure_optimizers(), 1, graph)
            for i in range(3):
                fast.step(batch, i)
            keep.append((m, fast))
            fns[name] = (lambda f: lambda: f.step(batch, 0))(fast)
        Linear.fwd_route, Linear.bwd_route = default_routes
        modes = {"replay": keep[0][1].mode, "eager_launches": keep[1][1].mode,
                 "default_routes": {"fwd": default_routes[0], "bwd": default_routes[1]}}
        if a.parent:
            torch.manual_seed(0)
            pm = _parent_vae(a.parent)(**cfg["model"]["args"]).to(dev)
            pm.train()
            popt = pm.configure_optimizers()

            def parent_step():
                loss = pm.training_step(batch, 0)
                loss.backward()
                popt.step()
                popt.zero_grad()
            fns["parent_commit"] = parent_step
            modes["parent_commit"] = f"eager ATen + {type(popt).__module__}.{type(popt).__name__}"
        t = alternate(torch, fns, a.runs, a.window)
        t["modes"] = modes
        if a.parent:
            t["parent_over_replay"] = round(t["parent_commit"] / t["replay"], 2)
        rec["train_step"][f"B{B}"] = t
        print(f"train step B{B}: {t}", flush=True)
        del keep, fns

    # (iii) bench.py, this tree against the parent's
    if a.parent and a.bench_rounds > 0:
        torch.cuda.synchronize()
        rec["bench"] = {}
        for wl in ("ddpm32", "vqvae"):
            got = {"this": [], "parent": []}
            for _ in range(a.bench_rounds):
                for who, cwd in (("this", here), ("parent", a.parent)):
                    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10", "--workload", wl,
                                        "--only", "--no-cpu-baseline", "--no-roofline"], cwd=cwd, capture_output=True, text=True,
                                       timeout=600)
                    if r.returncode != 0:
                        raise SystemExit(f"bench.py ({who}, {wl}) failed:\n{r.stderr[-2000:]}")
                    got[who].append(_bench_line(r.stdout)["value"])
            med = {k: statistics.median(v) for k, v in got.items()}
            rec["bench"][wl] = {"images_per_s": got, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4)}
            print(f"bench {wl}: {rec['bench'][wl]}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
