"""Measure the denoising autoencoder on the HIP path -> profiles/r25_dae_bench.json.  Needs a GPU; nothing falls back.

  (i)   the corruption and loss launches of csrc/dae.hip alone, on the shapes of configs/autoencoder/dae.json at B = 32 and
        B = 256: median of ``--runs`` alternating windows of ``--window`` calls between device events, and their share of the
        eager step's time;
  (ii)  the training step at B = 32 (the config) and B = 256: graph replay, the same step object issuing eager launches, the
        replayed step under every other (fwd, bwd) route of ``lgm_hip.nn.Linear``, the replayed step of the two mask modes, and
        the same network from plain torch layers (``nn.Linear``, autograd) with ``torch.optim.Adam`` on the same device, the
        candidates taking turns;
  (iii) with ``--parent DIR`` (a checkout of the parent commit, its library built): ``bench.py`` on this tree and on the
        parent's, alternating, ``--bench-rounds`` times each.
TIME ONLY: the networks are untrained.

Usage:  python tools/dae_bench.py [--parent DIR] [--bench-rounds N]
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


def plain_torch_step(torch, dev, B):
    """the reference's network from torch's own layers, autograd and Adam, on the device"""
    nn = torch.nn
    enc = nn.Sequential(nn.Linear(784, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU())
    dec = nn.Sequential(nn.Linear(128, 256), nn.ReLU(), nn.Linear(256, 784), nn.Tanh())
    net = nn.Sequential(enc, dec).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    metric = nn.MSELoss()

    def step(batch):
        x = batch[0]
        noisy = x + torch.randn_like(x) * 0.1
        loss = metric(x, net(noisy.view(B, -1)).view_as(x))
        loss.backward()
        opt.step()
        opt.zero_grad()
    return step


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r25_dae_bench.json"))
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
    cfg = load_config(os.path.join(here, "lightning-generative-models_amd", "configs", "autoencoder", "dae.json"))
    D = 784

    # (i) the launches of csrc/dae.hip, alone
    for B in (32, 256):
        gen = torch.Generator().manual_seed(B)
        x, noise = (torch.rand(B, D, generator=gen) * 2 - 1).to(dev), torch.randn(B, D, generator=gen).to(dev)
        pre = torch.randn(B, D, generator=gen).to(dev)
        key = torch.tensor([12345], dtype=torch.int64, device=dev)
        out, xh, gpre = (torch.empty(B, D, device=dev) for _ in range(3))
        row, vals, gl = torch.empty(B, device=dev), torch.empty(1, device=dev), torch.ones(1, device=dev)
        t = alternate(torch, {
            "dae_corrupt": lambda: ops.dae_corrupt(x, noise, 0.1, out),
            "dae_corrupt_mask salt_and_pepper": lambda: ops.dae_corrupt_mask(x, key, "salt_and_pepper", 0.1, out),
            "dae_corrupt_mask masking": lambda: ops.dae_corrupt_mask(x, key, "masking", 0.1, out),
            "randn [B, D] (torch)": lambda: torch.randn([B, D], device=dev),
            "key.random_ (torch)": lambda: key.random_(-2 ** 63, None),
            "dae_tanh_mse_fwd": lambda: ops.dae_tanh_mse_fwd(pre, x, D, xh, row),
            "dae_tanh_mse_bwd": lambda: ops.dae_tanh_mse_bwd(xh, x, gl, D, gpre),
            "dae_loss": lambda: ops.dae_loss(row, D, vals)}, a.runs, a.window)
        rec["kernels"][f"corruption and loss B{B}"] = t
        print(f"corruption and loss B{B}: {t}", flush=True)

    # (ii) the training step
    rec["train_step"] = {}
    for B in (32, 256):
        img = torch.rand(B, 1, 28, 28, device=dev) * 2 - 1
        batch = (img, None)
        fns, keep = {}, []
        default_routes = (Linear.fwd_route, Linear.bwd_route)
        variants = [("replay", True, default_routes, "gaussian"), ("eager_launches", False, default_routes, "gaussian")]
        variants += [(f"replay fwd={f} bwd={b_}", True, (f, b_), "gaussian") for f in ("dense", "generic")
                     for b_ in ("dense", "generic") if (f, b_) != default_routes]
        variants += [(f"replay {nt}", True, default_routes, nt) for nt in ("salt_and_pepper", "masking")]
        for name, graph, routes, nt in variants:         # a model and a captured step per variant: the routes are baked in
            Linear.fwd_route, Linear.bwd_route = routes
            torch.manual_seed(0)
            m = load_model({"name": "DAE", "args": dict(cfg["model"]["args"], noise_type=nt)}).to(dev)
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
        pstep = plain_torch_step(torch, dev, B)
        fns["plain_torch_adam"] = lambda: pstep(batch)
        modes["plain_torch_adam"] = "nn.Linear layers, autograd, torch.optim.Adam"
        t = alternate(torch, fns, a.runs, a.window)
        t["modes"] = modes
        t["eager_over_replay"] = round(t["eager_launches"] / t["replay"], 2)
        t["plain_torch_over_replay"] = round(t["plain_torch_adam"] / t["replay"], 2)
        k = rec["kernels"][f"corruption and loss B{B}"]
        own = k["dae_corrupt"] + k["dae_tanh_mse_fwd"] + k["dae_tanh_mse_bwd"] + k["dae_loss"]
        t["dae_hip_launches_alone_us"] = round(own, 2)
        t["dae_hip_share_of_eager_step"] = round(own / t["eager_launches"], 3)
        rec["train_step"][f"B{B}"] = t
        print(f"train step B{B}: {t}", flush=True)
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
        med = {k: statistics.median(v) for k, v in got.items()}
        rec["bench"] = {"value": got, "median": med, "this_over_parent": round(med["this"] / med["parent"], 4),
                        "parent_spread": round((max(got["parent"]) - min(got["parent"])) / med["parent"], 4)}
        print(f"bench: {rec['bench']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
