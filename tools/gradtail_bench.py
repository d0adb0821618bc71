"""Time the gradient tail - global-norm clipping and gradient accumulation - on the graph-replayed DDPM step, one GPU.

DDPM 32 x 32 (UNet dim 64, random weights and data), ``DDPMFastStep`` in graph-replay mode.  Every figure is the median over
``--runs`` windows (``torch.cuda.synchronize`` on both sides of a window of ``--window`` optimizer steps) after warm-up, the
variants of one comparison alternating window by window inside one process:

  (i)   the plain step at B = 128 - with ``--tree DIR --parent-only`` the same on another checkout (the parent commit with its
        own library), whose result file ``--parent FILE ...`` puts beside this commit's: the default path must not have moved;
  (ii)  the same step with ``max_grad_norm`` set, beside the launches it adds timed alone (device events around back-to-back
        launches on the model's own flat buffers) and the byte floor of one 4 B/parameter read at the streaming rate
        ``ema_lerp`` (12 B/parameter) reaches in the same process;
  (iii) accumulate_grad_batches = 4 at micro-batch 32: ms per OPTIMIZER step on the fast path, beside the slow path of the
        same checkout (training_step / (loss / K).backward() launch by launch, what the parent commit runs for K > 1) and
        the accumulate pass alone beside its 12 B/parameter.

Usage:  python tools/gradtail_bench.py [--out profiles/r14_gradtail_bench.json] [--parent FILE ...] [--base FILE]
        python tools/gradtail_bench.py --tree DIR --parent-only --out FILE
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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r14_gradtail_bench.json"))
    ap.add_argument("--parent", default=None, nargs="*", help="result files of --parent-only runs on the parent commit")
    ap.add_argument("--parent-only", action="store_true", help="only what another checkout can run: (i) and the slow path of (iii)")
    ap.add_argument("--base", default=None, help="measure nothing: start from this result file and apply --parent")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5, help="optimizer steps per timed window")
    a = ap.parse_args()
    out = json.load(open(a.base)) if a.base else measure(a, here)
    if a.parent:
        bases = [json.load(open(f)) for f in a.parent]
        out["parent_commit"] = [{k: b[k] for k in ("plain_step_ms", "slow_accumulate_step_ms")} for b in bases]
        plain = statistics.median(b["plain_step_ms"] for b in bases)
        slow = statistics.median(b["slow_accumulate_step_ms"] for b in bases)
        out["plain_step_over_parent"] = round(out["plain_step_ms"] / plain, 4)
        out["accumulate_step_parent_over_fast"] = round(slow / out["accumulate_step_ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def measure(a, here):
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion.ddpm import DDPM
    assert torch.cuda.is_available(), "gradtail_bench needs a GPU: it does not fall back"
    dev = torch.device("cuda", 0)
    K, MICRO, FULL = 4, 32, 128

    def module():
        torch.manual_seed(0)
        m = DDPM(img_channels=3, img_size=32, dim=64, lr=8e-5)
        m.sample_every = 0
        m.to(dev)
        m.prepare_hip(dev)
        m.train()
        return m, m.configure_optimizers()

    g = torch.Generator().manual_seed(1)
    x_full = (torch.rand(FULL, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    x_micro = x_full[:MICRO].contiguous()

    def fast_steps(fast, x, micro_per_step):
        def run(n):
            for i in range(n * micro_per_step):
                fast.step((x, None), i)
        return run

    def slow_steps(m, opt, x):
        """MiniTrainer's loop for accumulate_grad_batches = K without a fast step object"""
        def run(n):
            for _ in range(n):
                for k in range(K):
                    (m.training_step((x, None)) / K).backward()
                    if k == K - 1:
                        opt.step()
                        opt.zero_grad()
                    m.on_train_batch_end(None, None, k)
        return run

    def timed(variants):
        """{name: run(n)} -> {name: ms per optimizer step}: warm-up, then a.runs windows per variant, alternating"""
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

    out = {"what": f"DDPM 32 x 32, UNet dim 64, one GPU, DDPMFastStep in graph-replay mode; ms per optimizer step: wall time of "
                   f"windows of {a.window} optimizer steps (torch.cuda.synchronize on both sides), median of {a.runs} windows "
                   f"after warm-up, the variants of one comparison alternating",
           "device": torch.cuda.get_device_name(0), "tree": "this commit" if root == here else "parent commit"}
    m0, o0 = module()
    plain = DDPMFastStep(m0, o0, 1, use_graph=True)
    variants = {"plain": fast_steps(plain, x_full, 1)}
    if not a.parent_only:
        m1, o1 = module()
        o1.max_grad_norm = 1.0
        clipped = DDPMFastStep(m1, o1, 1, use_graph=True)
        variants["clipped"] = fast_steps(clipped, x_full, 1)
    ms, windows = timed(variants)
    assert plain.mode.startswith("hipGraph"), "graph replay is unavailable: the figures would be eager launches"
    out["plain_step_ms"], out["windows_ms"] = ms["plain"], windows
    if not a.parent_only:
        out["clipped_step_ms"] = ms["clipped"]
    n_param = m0.ema.online_model.model._flat.total
    out["parameters"] = n_param

    ms2, s = module()
    variants = {"slow": slow_steps(ms2, s, x_micro)}
    if not a.parent_only:
        m3, o3 = module()
        accum = DDPMFastStep(m3, o3, 1, use_graph=True, accumulate=K)
        variants["fast"] = fast_steps(accum, x_micro, K)
    ms, windows = timed(variants)
    out["slow_accumulate_step_ms"] = ms["slow"]
    out["windows_accumulate_ms"] = windows
    if a.parent_only:
        return out
    assert clipped.mode.startswith("hipGraph") and accum.mode.startswith("hipGraph")
    out["clip_added_us"] = round((out["clipped_step_ms"] - out["plain_step_ms"]) * 1e3, 1)
    out["accumulate_step_ms"] = ms["fast"]
    out["accumulate"] = {"K": K, "micro_batch": MICRO, "slow_over_fast_same_checkout": round(ms["slow"] / ms["fast"], 3)}

    def alone(fn, n=200):
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

    fp, fe = m1.ema.online_model.model._flat, m1.ema.ema_model.model._flat
    partials = torch.empty(ops.grad_sqnorm_partials(n_param), dtype=torch.float64, device=dev)
    out2 = torch.empty(2, device=dev)
    acc = torch.empty_like(fp.grad)
    us = {"sqnorm_partial": alone(lambda: ops.grad_sqnorm_partial(fp.grad, partials)),
          "clip_scale": alone(lambda: ops.grad_clip_scale(partials, 1.0, 1.0, out2)),
          "ema_lerp": alone(lambda: ops.ema_lerp(fe.data, fp.data, 0.5)),
          "grad_accumulate": alone(lambda: ops.grad_accumulate(acc, fp.grad)),
          "grad_accumulate_overwrite": alone(lambda: ops.grad_accumulate(acc, fp.grad, overwrite=True))}
    rate = 12.0 * n_param / us["ema_lerp"]                     # bytes per microsecond
    out["launch_alone_us"] = us
    out["streaming"] = {
        "ema_lerp_GBps": round(rate * 1e-3, 1),
        "sqnorm_partial_GBps": round(4.0 * n_param / us["sqnorm_partial"] * 1e-3, 1),
        "grad_accumulate_GBps": round(12.0 * n_param / us["grad_accumulate"] * 1e-3, 1),
        "sqnorm_floor_us_at_ema_rate": round(4.0 * n_param / rate, 2),
        "accumulate_floor_us_at_ema_rate": round(12.0 * n_param / rate, 2),
        "partials": partials.numel(), "span": ops.grad_sqnorm_span(n_param)}
    # the pass reads 4 B/parameter and does one double FMA per element: it is bound by the reads when it reaches the byte rate
    # of a pass that does no double arithmetic at all
    out["streaming"]["sqnorm_bound_by"] = ("memory reads" if out["streaming"]["sqnorm_partial_GBps"] >= 0.8 * out["streaming"]["ema_lerp_GBps"]
                                           else "below 0.8 of the streaming rate: FP64 adds or launch latency")
    print(json.dumps({k: out[k] for k in ("launch_alone_us", "streaming")}), flush=True)
    return out


if __name__ == "__main__":
    main()
