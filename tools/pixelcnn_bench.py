"""Measure the gated PixelCNN prior at its working size -> profiles/r22_pixelcnn_bench.json.  Needs a GPU; nothing falls back.

  (i)   each masked kernel (lgm_mconv_xy / _yx / _wgrad) on the two layer shapes of configs/vae/vqvae_prior.json (B = 256, 8 x 8
        codes: 64 -> 128 type A, 128 -> 256 type B, k = 7) beside the generic entry point (lgm_conv_xy / _yx / _wgrad through
        lgm_hip.ops) on the SAME zero-masked weights, in the same process: median of ``--runs`` alternating windows of
        ``--window`` calls between device events;
  (ii)  ``sample(64)`` (h w graph-replayed incremental steps + the VQ-VAE's decoder) beside a loop of h w full forwards of the
        same batch (the reference's way, without its draw);
  (iii) the prior's graph-replayed training step at B = 256 (the frozen VQ-VAE's encoder included), under both backward routes
        (``MaskedConv2d.backward_route``).
TIME ONLY: the networks are untrained.  ``--bench FILE ...``: files holding bench.py's JSON result line, copied into the record
under the file's name.

Usage:  python tools/pixelcnn_bench.py [--bench FILE ...]
"""
import argparse
import ctypes
import json
import os
import statistics
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


def _bench_line(path):
    for ln in reversed(open(path).read().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit(f"{path} holds no JSON result line")


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r22_pixelcnn_bench.json"))
    ap.add_argument("--bench", default=None, nargs="*")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=10)
    a = ap.parse_args()
    for p in (here, os.path.join(here, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops
    from models.generative.autoregressive.pixelcnn import PixelCNN, live_taps
    from utils.loader import load_config, load_model
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    L = ops.lib()
    st = ops.stream
    rec = {"runs": a.runs, "window": a.window, "unit": "us per call, median of alternating windows", "kernels": {}}

    # (i) kernels
    B, H, W, k = 256, 8, 8, 7
    for C, N, mt in ((64, 128, "A"), (128, 256, "B")):
        Lv = live_taps(k, mt)
        g = ops.make_geom(B, H, W, C, N, k, k, 1, k // 2)
        gen = torch.Generator().manual_seed(C)
        w = torch.randn(N, k * k, C, generator=gen).to(dev) / (Lv * C) ** 0.5
        w[:, Lv:, :] = 0                                          # the generic kernels multiply these zeros
        bias = torch.randn(N, generator=gen).to(dev)
        x, gy = torch.randn(B, H, W, C, generator=gen).to(dev), torch.randn(B, H, W, N, generator=gen).to(dev)
        y, gx = torch.empty_like(gy), torch.empty_like(x)
        gw, gb = torch.empty_like(w), torch.empty_like(bias)
        gw2, gb2 = torch.empty_like(w), torch.empty_like(bias)
        gp = ctypes.byref(g)
        wneed = L.lgm_mconv_wgrad_workspace(gp, Lv)
        wws = torch.empty(max(wneed // 4, 4), device=dev)
        cases = {
            "xy": {"masked": lambda: L.lgm_mconv_xy(gp, Lv, x.data_ptr(), C, w.data_ptr(), bias.data_ptr(), y.data_ptr(), N, st()),
                   "generic": lambda: ops.conv_xy(g, x, w.data_ptr(), bias.data_ptr(), None, y)},
            "yx": {"masked": lambda: L.lgm_mconv_yx(gp, Lv, gy.data_ptr(), N, w.data_ptr(), None, 0, gx.data_ptr(), C, st()),
                   "generic": lambda: ops.conv_yx(g, gy, w.data_ptr(), None, None, gx)},
            "wgrad": {"masked": lambda: L.lgm_mconv_wgrad(gp, Lv, gy.data_ptr(), N, x.data_ptr(), C, gw.data_ptr(), gb.data_ptr(),
                                                         0.0, wws.data_ptr(), wneed, st()),
                      "generic": lambda: ops.conv_wgrad(g, gy, x, gw2.data_ptr(), 0.0, gb2.data_ptr())},
        }
        flop = 2.0 * B * H * W * C * N
        for name, fns in cases.items():
            t = alternate(torch, fns, a.runs, a.window)
            t["live_taps"], t["taps"] = Lv, k * k
            t["masked_tflops_live"] = round(flop * Lv / t["masked"] / 1e6, 2)
            t["generic_tflops_all_taps"] = round(flop * k * k / t["generic"] / 1e6, 2)
            t["masked_over_generic"] = round(t["masked"] / t["generic"], 3)
            rec["kernels"][f"{name} {C}->{N} {mt}"] = t
            print(f"{name} {C}->{N} {mt}: {t}", flush=True)
        # the same result on the same weights (reordered sums)
        L.lgm_mconv_xy(gp, Lv, x.data_ptr(), C, w.data_ptr(), bias.data_ptr(), y.data_ptr(), N, st())
        y2 = torch.empty_like(y)
        ops.conv_xy(g, x, w.data_ptr(), bias.data_ptr(), None, y2)
        rec["kernels"][f"xy {C}->{N} {mt}"]["rel_diff_masked_vs_generic"] = float((y - y2).norm() / y2.norm())

    # (ii) sampling, (iii) the training step
    cfg = load_config(os.path.join(here, "lightning-generative-models_amd", "configs", "vae", "vqvae_prior.json"))
    torch.manual_seed(0)
    net = load_model(cfg["model"])
    assert isinstance(net, PixelCNN)
    net.to(dev)
    net.prepare_hip(dev)
    h, w_ = net.grid
    q = torch.randn(64, net.input_channels, h, w_, device=dev)

    def full_forwards():
        with torch.no_grad():
            for _ in range(h * w_):
                net(q)
    rec["sample64"] = alternate(torch, {"incremental_sample": lambda: net.sample(64), "hw_full_forwards": full_forwards},
                                a.runs, 2)
    rec["sample64"]["unit"] = "us per batch of 64 images"
    rec["sample64"]["positions"] = h * w_
    print("sample64:", rec["sample64"], flush=True)
    from models.generative.autoregressive.pixelcnn import MaskedConv2d
    img = torch.rand(256, 3, 64, 64, device=dev)
    rec["train_step_b256"] = {"default_backward_route": MaskedConv2d.backward_route}
    for route in ("generic", "masked"):                           # a model and a captured step per route
        MaskedConv2d.backward_route = route
        torch.manual_seed(0)
        m = load_model(cfg["model"]).to(dev)
        m.train()
        fast = m.make_fast_step(m.configure_optimizers(), 1, True)
        for i in range(3):
            fast.step((img, None), i)
        rec["train_step_b256"][route] = {"us": alternate(torch, {"step": lambda: fast.step((img, None), 0)}, a.runs,
                                                         a.window)["step"], "mode": fast.mode}
        del fast, m
    MaskedConv2d.backward_route = rec["train_step_b256"]["default_backward_route"]
    print("train step:", rec["train_step_b256"], flush=True)
    for p in a.bench or []:
        rec.setdefault("bench", {})[os.path.basename(p)] = _bench_line(p)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
