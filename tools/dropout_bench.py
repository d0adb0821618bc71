"""Time dropout (``DDPM(dropout=p)``) on the DDPM training step and on the GroupNorm launches that carry it, one GPU.

DDPM 32 x 32 (UNet dim 64, random weights and data), B = 128, graph replay.  Step figures are the median over ``--runs`` windows
(``torch.cuda.synchronize`` on both sides of a window of ``--window`` steps) after warm-up, the variants of one process
alternating window by window, as tools/tsampler_bench.py does:

  (i)   the plain step on this tree and, with ``--parent-tree DIR``, on another checkout (the parent commit with its own
        library): fresh child processes started from this call, alternating tree by tree, ``--rounds`` each - the shared
        kernel bodies of csrc/norm.hip must not have moved the default path;
  (ii)  the step with ``dropout = 0.1`` beside the plain one in one process, with the library calls of one eager step of each
        (by entry point), the GroupNorm plans of the 19 ``block1`` norms and the launches the key draw adds;
  (iii) between device events, back-to-back launches: the one-pass GroupNorm forward (FiLM + SiLU) and backward with and without
        the mask at (B, C, H, W, G) = (128, 64, 32, 32, 8) and (128, 512, 4, 4, 8), and the stand-alone pair at the same shapes;
  (iv)  ``--bench FILE ...`` / ``--bench-parent FILE ...``: bench.py's result lines on both trees, copied in.

Usage:  python tools/dropout_bench.py [--parent-tree DIR] [--out profiles/r17_dropout_bench.json] [--bench FILE ...]
"""
import argparse
import ctypes
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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r17_dropout_bench.json"))
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, built: (i) alternates with it")
    ap.add_argument("--plain-only", action="store_true", help="child mode: the plain step of --tree alone, JSON on stdout")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench", default=None, nargs="*", help="files holding bench.py's JSON result line, this commit")
    ap.add_argument("--bench-parent", default=None, nargs="*", help="the same from the parent commit's tree")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    a = ap.parse_args()
    if a.plain_only:
        print("RESULT " + json.dumps(measure(a, here, plain_only=True)))
        return
    out = {}
    if a.parent_tree:
        rounds = {"this commit": [], "parent commit": []}
        for _ in range(a.rounds):
            for name, tree in (("parent commit", a.parent_tree), ("this commit", here)):
                rounds[name].append(_child(a, tree)["plain_step_ms"])
        out["plain_step_ms_by_tree"] = rounds
        out["plain_step_over_parent"] = round(statistics.median(rounds["this commit"]) / statistics.median(rounds["parent commit"]), 4)
    out.update(measure(a, here, plain_only=False))
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


def measure(a, here, plain_only):
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import _lib, ops
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion import ddpm as D
    assert torch.cuda.is_available(), "dropout_bench needs a GPU: it does not fall back"
    assert os.path.abspath(_lib.LIB_PATH).startswith(root), f"library {_lib.LIB_PATH} is not the one of {root}"
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

    steps = {"plain": DDPMFastStep(*module(), 1, use_graph=True)}
    if plain_only:
        ms, windows = timed({k: fast_steps(f) for k, f in steps.items()})
        assert steps["plain"].mode.startswith("hipGraph")
        return {"tree": root, "plain_step_ms": ms["plain"], "windows_ms": windows["plain"]}
    out = {"what": f"DDPM 32 x 32, UNet dim 64, B = {FULL}, one GPU, graph replay; ms per step: wall time of windows of "
                   f"{a.window} steps (torch.cuda.synchronize on both sides), median of {a.runs} windows after warm-up, the "
                   f"variants of one process alternating; us figures: 200 back-to-back launches between two device events",
           "device": torch.cuda.get_device_name(0)}
    steps["dropout_0.1"] = DDPMFastStep(*module(dropout=0.1), 1, use_graph=True)
    ms, windows = timed({k: fast_steps(f) for k, f in steps.items()})
    for k, f in steps.items():
        assert f.mode.startswith("hipGraph"), f"{k}: graph replay is unavailable, the figures would be eager launches"
    out["step_ms"], out["windows_ms"] = ms, windows
    out["dropout_added_us"] = round((ms["dropout_0.1"] - ms["plain"]) * 1e3, 1)

    # ---- the library calls of one eager step, by entry point (a fused variant REPLACES its plain call: the counts must agree)
    def calls_of(**kw):
        m, opt = module(**kw)
        fast = DDPMFastStep(m, opt, 1, use_graph=False)
        fast.step((x_full, None), 0)                       # allocations, plans
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
            fast.step((x_full, None), 1)
        finally:
            for name, fn in saved.items():
                setattr(L, name, fn)
        torch.cuda.synchronize()
        return seen
    plain_calls, drop_calls = calls_of(), calls_of(dropout=0.1)
    host_tails = ("_supported", "_workspace", "_workspaces", "_workspace_partial", "_fits", "_floats", "_preferred", "_slabs", "_span",
                  "_partials")
    host_names = {"lgm_abi_version", "lgm_cu_margin", "lgm_set_cu_margin", "lgm_gn_plan", "lgm_kernel_name", "lgm_kernel_name_count",
                  "lgm_last_error", "lgm_last_kernel", "lgm_wgrad_queue_enable", "lgm_wino4_set_debug_buffer", "lgm_wino4_set_light",
                  "lgm_wino_set_debug_buffer"}
    launching = lambda c: {k: v for k, v in c.items() if not k.endswith(host_tails) and k not in host_names}      # noqa: E731
    pc, dc = launching(plain_calls), launching(drop_calls)
    out["library_calls_one_eager_step"] = {
        "plain": sum(pc.values()), "dropout_0.1": sum(dc.values()),
        "entry points whose count differs": {k: [pc.get(k, 0), dc.get(k, 0)] for k in sorted(set(pc) | set(dc)) if pc.get(k, 0) != dc.get(k, 0)}}
    net = steps["dropout_0.1"].net
    plans, res = [], 32
    shapes = []
    for s, (b1, b2, _, _) in enumerate(net.downs):
        shapes += [(b1.dim_out, res), (b2.dim_out, res)]
        res = res if s == len(net.downs) - 1 else res // 2
    shapes += [(net.mid_block1.dim_out, res), (net.mid_block2.dim_out, res)]
    for u, (b1, b2, _, _) in enumerate(net.ups):
        shapes += [(b1.dim_out, res), (b2.dim_out, res)]
        res = res if u == len(net.ups) - 1 else res * 2
    shapes.append((net.final_res_block.dim_out, res))
    for C, r in shapes:
        cb, nt, nv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ops.lib().lgm_gn_plan(FULL, r * r, C, 8, 0, ctypes.byref(cb), ctypes.byref(nt), ctypes.byref(nv))
        plans.append({"C": C, "HW": r * r, "cb": cb.value, "nt": nt.value, "nv": nv.value})
    out["block1_norm_plans"] = plans
    out["block1_norms_on_two_pass_plans"] = sum(1 for p in plans if p["nv"] == 0)
    out["launches_added_per_step"] = {"key draw (torch random_ on one int64)": 1,
                                      "stand-alone dropout kernels (forward + backward)": 2 * out["block1_norms_on_two_pass_plans"]}

    # ---- (iii) the GroupNorm launches alone
    L, st = ops.lib(), ops.stream()
    keyt = torch.tensor([0x1234ABCD9E3779B], dtype=torch.int64, device=dev)
    thr, scale = ops.dropout_operands(0.1)
    drop = (keyt.data_ptr(), 3, 0, thr, scale)
    alone_us = {}
    for (B, C, H, W, G) in ((128, 64, 32, 32, 8), (128, 512, 4, 4, 8)):
        P = H * W
        gg = torch.Generator().manual_seed(C)
        r = lambda *s: torch.randn(*s, generator=gg).to(dev)      # noqa: E731
        x, gy, ss, gamma, beta = r(B * P, C), r(B * P, C), 0.5 * r(B, 2 * C), 1 + 0.3 * r(C), 0.2 * r(C)
        y, gx = torch.empty_like(x), torch.empty_like(x)
        mean, rstd, A, Bc = torch.empty(B * G, device=dev), torch.empty(B * G, device=dev), torch.empty(B * C, device=dev), torch.empty(B * C, device=dev)
        gg_, gb_, gss, ws = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty(B, 2 * C, device=dev), torch.empty(5 * B * C, device=dev)
        cb, nt, nv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.lgm_gn_plan(B, P, C, G, 0, ctypes.byref(cb), ctypes.byref(nt), ctypes.byref(nv))
        assert nv.value > 0, "a one-pass plan was expected"
        ftail = (B, P, C, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), ss.data_ptr(), 2 * C, 1, None, 0, y.data_ptr(), C, mean.data_ptr(),
                 rstd.data_ptr(), A.data_ptr(), Bc.data_ptr())
        bmid = (B, P, C, G, gamma.data_ptr(), beta.data_ptr(), ss.data_ptr(), 2 * C, 1, mean.data_ptr(), rstd.data_ptr(), A.data_ptr(),
                Bc.data_ptr(), gx.data_ptr(), C, 0, gg_.data_ptr(), gb_.data_ptr(), 0.0, gss.data_ptr(), 2 * C, 0.0, ws.data_ptr())
        gyw = gy.clone()
        alone_us[f"{B}x{C}x{H}x{W}x{G} plan ({cb.value}, {nt.value}, {nv.value})"] = {
            "gn_fwd_us": alone(torch, lambda: L.lgm_gn_fwd(x.data_ptr(), C, *ftail, st)),
            "gn_fwd_drop_us": alone(torch, lambda: L.lgm_gn_fwd_drop(None, 0, 0, None, x.data_ptr(), C, *ftail, *drop, st)),
            "gn_bwd_us": alone(torch, lambda: L.lgm_gn_bwd(x.data_ptr(), C, gy.data_ptr(), C, *bmid, st)),
            "gn_bwd_drop_us": alone(torch, lambda: L.lgm_gn_bwd_drop(x.data_ptr(), C, gy.data_ptr(), C, None, 0, 0, *bmid, None, None, *drop, st)),
            "dropout_fwd_alone_us": alone(torch, lambda: L.lgm_dropout_fwd(y.data_ptr(), C, B, P, C, *drop, st)),
            "dropout_bwd_alone_us": alone(torch, lambda: L.lgm_dropout_bwd(gyw.data_ptr(), C, B, P, C, *drop, st))}
    out["groupnorm_launches_alone"] = alone_us
    return out


if __name__ == "__main__":
    main()
