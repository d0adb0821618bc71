"""Measure the NICE flow on the HIP path -> profiles/r26_nice_bench.json.  Needs a GPU; nothing falls back.

  (i)   the launches of csrc/nice.hip alone, on the shapes of configs/flow/nice.json at B = 32 and B = 256: median of ``--runs``
        alternating windows of ``--window`` calls between device events, and their share of the eager step's time;
  (ii)  the training step at B = 32 (the config) and B = 256: graph replay, the same step object issuing eager launches, the
        replayed step under every other (fwd, bwd) route of ``lgm_hip.nn.Linear``, and the same module's plain-torch layers
        (``CouplingLayer.forward``: slices, ``F.linear``, cat; autograd) with ``torch.optim.Adam`` on the same device, the
        candidates taking turns;
  (iii) with ``--parent DIR`` (a checkout of the parent commit, its library built): ``bench.py`` on this tree and on the
        parent's, alternating, ``--bench-rounds`` times each.
TIME ONLY: the networks are untrained.

Usage:  python tools/nice_bench.py [--parent DIR] [--bench-rounds N]
"""
import argparse
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
    """{name: median us per call} over ``runs`` windows of ``n`` calls each, the candidates taking turns; the smallest and the
    largest window of every candidate under "windows_min_max": two medians closer than that are a tie"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            got[k].append(window(torch, fn, n))
    out = {k: round(statistics.median(v), 2) for k, v in got.items()}
    out["windows_min_max"] = {k: [round(min(v), 2), round(max(v), 2)] for k, v in got.items()}
    return out


def _bench_line(text):
    for ln in reversed(text.splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("bench.py printed no JSON result line")


def plain_torch_step(torch, m):
    """the module's own plain-torch layers (what it runs on a CPU device), autograd and Adam, on the GPU"""
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    def step(batch):
        x = batch[0].view(batch[0].shape[0], -1)
        h = x
        for layer in m.layers:
            h = layer(h)
        loss = -m._compute_loss(m.scaling_layer(h), x)
        loss.backward()
        opt.step()
        opt.zero_grad()
    return step


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r26_nice_bench.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (bench.py needs its library built)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=20)
    a = ap.parse_args()
    for p in (here, os.path.join(here, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops
    from lgm_hip.nn import Linear
    from utils.loader import load_config, load_model
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    rec = {"runs": a.runs, "window": a.window, "unit": "us per call, median of alternating windows", "kernels": {}}
    cfg = load_config(os.path.join(here, "lightning-generative-models_amd", "configs", "flow", "nice.json"))
    D, half = 784, 392

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)

    # (i) the launches of csrc/nice.hip, alone
    for B in (32, 256):
        gen = torch.Generator().manual_seed(B)
        x, t = (torch.rand(B, D, generator=gen) * 2 - 1).to(dev), torch.randn(B, half, generator=gen).to(dev)
        ls = (0.3 * torch.randn(D, generator=gen)).to(dev)
        out, z, gh = (torch.empty(B, D, device=dev) for _ in range(3))
        row, vals, gl, gls = torch.empty(B, device=dev), torch.empty(3, device=dev), torch.ones(1, device=dev), torch.zeros(D, device=dev)
        ops.nice_scale_fwd(x, ls.data_ptr(), D, False, z, row)
        tk = alternate(torch, {
            "nice_couple": lambda: ops.nice_couple(x, t, half, 1, out),
            "nice_couple in place": lambda: ops.nice_couple(out, t, 0, 1, out),
            "nice_scale_fwd": lambda: ops.nice_scale_fwd(x, ls.data_ptr(), D, False, z, row),
            "nice_scale_fwd reverse, no row_part": lambda: ops.nice_scale_fwd(x, ls.data_ptr(), D, True, z, None),
            "nice_loss": lambda: ops.nice_loss(row, ls.data_ptr(), D, True, vals),
            "nice_scale_bwd": lambda: ops.nice_scale_bwd(z, ls.data_ptr(), gl, D, True, gh, gls.data_ptr(), 0.0)}, a.runs, a.window)
        rec["kernels"][f"B{B}"] = tk
        print(f"kernels B{B}: {tk}", flush=True)
        save()

    # (ii) the training step
    rec["train_step"] = {}
    for B in (32, 256):
        img = torch.rand(B, 1, 28, 28, device=dev) * 2 - 1
        batch = (img, None)
        fns, keep = {}, []
        default_routes = (Linear.fwd_route, Linear.bwd_route)
        variants = [("replay", True, default_routes), ("eager_launches", False, default_routes)]
        variants += [(f"replay fwd={f} bwd={b_}", True, (f, b_)) for f in ("dense", "generic") for b_ in ("dense", "generic")
                     if (f, b_) != default_routes]
        for name, graph, routes in variants:            # a model and a captured step per variant: the routes are baked in
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
        torch.manual_seed(0)
        pstep = plain_torch_step(torch, load_model(cfg["model"]).to(dev))
        fns["plain_torch_adam"] = lambda: pstep(batch)
        modes["plain_torch_adam"] = "the module's plain-torch layers, autograd, torch.optim.Adam"
        ts = alternate(torch, fns, a.runs, a.window)
        ts["modes"] = modes
        ts["eager_over_replay"] = round(ts["eager_launches"] / ts["replay"], 2)
        ts["plain_torch_over_replay"] = round(ts["plain_torch_adam"] / ts["replay"], 2)
        k = rec["kernels"][f"B{B}"]
        L = len(keep[0][0].layers)
        own = 2 * L * k["nice_couple"] + k["nice_scale_fwd"] + k["nice_loss"] + k["nice_scale_bwd"]
        ts["nice_hip_launches_alone_us"] = round(own, 2)
        ts["nice_hip_share_of_eager_step"] = round(own / ts["eager_launches"], 3)
        rec["train_step"][f"B{B}"] = ts
        print(f"train step B{B}: {ts}", flush=True)
        save()
        del keep, fns

    # (iii) bench.py, this tree against the parent's
    if a.parent and a.bench_rounds > 0:
        torch.cuda.synchronize()
        got = {"this": [], "parent": []}
        for _ in range(a.bench_rounds):
            for who, cwd in (("parent", a.parent), ("this", here)):
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=cwd,
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"bench.py ({who}) failed:\n{r.stderr[-2000:]}")
                got[who].append(_bench_line(r.stdout)["value"])
                print(f"bench.py {who}: {got[who][-1]}", flush=True)
        med = {k: statistics.median(v) for k, v in got.items()}
        rec["bench"] = {"value": got, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4),
                        "parent_spread": round((max(got["parent"]) - min(got["parent"])) / med["parent"], 4)}
        print(f"bench: {rec['bench']}", flush=True)
    save()
    print(a.out)


if __name__ == "__main__":
    main()
