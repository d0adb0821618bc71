"""Measure DDIM inversion and the slerp launches -> profiles/r20_edit_bench.json.  Needs a GPU; nothing falls back.

  (i)   the plain 32 x 32 training step of THIS tree and of the parent commit's tree (``--parent-tree``, built), each in fresh
        processes, alternating: the editing calls add nothing to a training step, so the two must sit inside the documented +-2 %;
  (ii)  64 images at 64 x 64, graph replay: one ``encode`` chain of 20 pairs beside one DDIM chain of 20 steps in the same
        process, alternating windows - both are one forward and one update launch per step, so the per-step times should agree;
  (iii) ``lgm_slerp`` alone between device events at [64, 3, 64, 64], [32, 3, 128, 128] and [8, 3, 256, 256], each beside a
        device copy of one operand in the same process, with the workgroups each launch has and its algorithmic bytes (the
        two launches read a and b twice and write out once: five operand-sized passes against the copy's two).

Usage:  python tools/edit_bench.py [--parent-tree DIR] [--bench FILE ...] [--bench-parent FILE ...]
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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r20_edit_bench.json"))
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, built: (i) alternates with it")
    ap.add_argument("--plain-only", action="store_true", help="child mode: the plain step of --tree alone, JSON on stdout")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench", default=None, nargs="*", help="files holding bench.py's JSON result line, this commit")
    ap.add_argument("--bench-parent", default=None, nargs="*", help="the same from the parent commit's tree")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    a = ap.parse_args()
    if a.plain_only:
        print("RESULT " + json.dumps(plain_step(a)))
        return
    out = {}
    if a.parent_tree:
        rounds = {"this commit": [], "parent commit": []}
        for _ in range(a.rounds):
            for name, tree in (("parent commit", a.parent_tree), ("this commit", here)):
                rounds[name].append(_child(a, tree)["plain_step_ms"])
        out["plain_32_step_ms_by_tree"] = rounds
        out["plain_32_step_over_parent"] = round(statistics.median(rounds["this commit"]) / statistics.median(rounds["parent commit"]), 4)
    out.update(measure(a))
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


def _import(tree):
    root = os.path.abspath(tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import _lib
    assert torch.cuda.is_available(), "edit_bench needs a GPU: it does not fall back"
    assert os.path.abspath(_lib.LIB_PATH).startswith(root), f"library {_lib.LIB_PATH} is not the one of {root}"
    return root, torch


def timed(torch, a, variants):
    """ms per window: median of ``a.runs`` windows per variant, the variants alternating, after a warm-up of each"""
    for run in variants.values():
        run()
    wall = {k: [] for k in variants}
    for _ in range(a.runs):
        for k, run in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: round(statistics.median(v), 4) for k, v in wall.items()}, {k: [round(t, 3) for t in v] for k, v in wall.items()}


def plain_step(a):
    root, torch = _import(a.tree)
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion import ddpm as D
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = D.DDPM(img_channels=3, img_size=32, dim=64, lr=8e-5)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    fast = DDPMFastStep(m, m.configure_optimizers(), 1, use_graph=True)
    x = torch.rand(128, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(dev)

    def window():
        for i in range(a.window):
            fast.step((x, None), i)
    ms, windows = timed(torch, a, {"plain": window})
    assert fast.mode.startswith("hipGraph")
    return {"tree": root, "plain_step_ms": round(ms["plain"] / a.window, 4), "windows_ms": [round(w / a.window, 3) for w in windows["plain"]]}


def measure(a):
    root, torch = _import(a.tree)
    from lgm_hip import ops
    from models.generative.diffusion import ddpm as D
    dev = torch.device("cuda", 0)
    out = {"what": f"one GPU; chains: wall time of one chain (torch.cuda.synchronize on both sides), median of {a.runs} chains per "
                   f"variant after warm-up, the variants of one process alternating; us figures: 200 back-to-back calls between "
                   f"two device events", "device": torch.cuda.get_device_name(0)}
    # ---- (ii) encode beside DDIM: 64 images at 64 x 64, UNet dim 64, graph replay, 20 steps each
    B, S, N = 64, 64, 20
    net = D.Unet(dim=64)
    gd = D.GaussianDiffusion(net, img_size=S, sampling_timesteps=N).to(dev)
    net.prepare_hip(dev)
    img = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        z = gd.encode(img, steps=N + 1)
        variants = {"encode, 20 pairs": lambda: gd.encode(img, steps=N + 1), "ddim sample, 20 steps": lambda: gd.sample(batch_size=B),
                    "decode, 21 steps, clip off": lambda: gd.decode(z, steps=N + 1, clip=False)}
        ms, windows = timed(torch, a, variants)
    steps = {"encode, 20 pairs": N, "ddim sample, 20 steps": N, "decode, 21 steps, clip off": N + 1}
    out["chains_64_at_64x64_ms"], out["chains_64_at_64x64_windows_ms"] = ms, windows
    out["chains_64_at_64x64_ms_per_step"] = {k: round(v / steps[k], 4) for k, v in ms.items()}
    out["encode_step_over_ddim_step"] = round(out["chains_64_at_64x64_ms_per_step"]["encode, 20 pairs"]
                                              / out["chains_64_at_64x64_ms_per_step"]["ddim sample, 20 steps"], 4)
    del gd, net
    # ---- (iii) lgm_slerp alone, beside a device copy of one operand
    span, res = ops.slerp_span(), {}
    for Bs, Ss in ((64, 64), (32, 128), (8, 256)):
        g = torch.Generator().manual_seed(3)
        x, y = (torch.randn(Bs, Ss, Ss, 4, generator=g).to(dev) for _ in range(2))
        o, dst = torch.empty_like(x), torch.empty_like(x)
        lam = torch.full((Bs,), 0.5, device=dev)
        parts = torch.empty(ops.slerp_partials(Bs, Ss * Ss), dtype=torch.float64, device=dev)
        xv, yv, ov = x[..., :3], y[..., :3], o[..., :3]
        px = x.numel() * 4
        s_us = alone(torch, lambda: ops.slerp(xv, yv, lam, out=ov, partials=parts))
        c_us = alone(torch, lambda: dst.copy_(x))
        wgs = Bs * -(-Ss * Ss // span)
        res[f"[{Bs}, 3, {Ss}, {Ss}]"] = {
            "slerp_us (two launches)": s_us, "copy_us (one operand, [B, H, W, 4] float32)": c_us, "slerp_over_copy": round(s_us / c_us, 3),
            "operand_bytes": px, "slerp_algorithmic_bytes (a and b twice, out once)": 5 * px, "copy_bytes (read and write)": 2 * px,
            "slerp_TB_per_s": round(5 * px / s_us * 1e-6, 3), "copy_TB_per_s": round(2 * px / c_us * 1e-6, 3),
            "spans_per_sample": -(-Ss * Ss // span), "workgroups_per_launch": wgs}
    out["slerp_alone"] = res
    return out


if __name__ == "__main__":
    main()
