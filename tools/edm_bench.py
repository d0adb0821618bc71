"""Measure what elucidated diffusion costs beside the discrete-time paths -> profiles/r21_edm_bench.json.  Needs a GPU; nothing
falls back.

  (i)   the EDM training step beside the plain DDPM step at 32 x 32, B = 128, one process, graph replay, alternating windows -
        the difference is the Fourier network's unfused time-embedding path and the other q_sample launch TOGETHER (the two
        are not separated);
  (ii)  one Heun step beside two DDIM steps and one Euler step beside one DDIM step at 64 images of 64 x 64 (per-step time of
        whole chains, graph replay);
  (iii) between device events, beside ``qsample_slice_kernel`` in the same process: ``lgm_edm_qsample``, the three sampling
        kernels, the Fourier forward and backward (launches issued from Python: launch-overhead bound at these sizes);
  (iv)  a 32-step Heun ``sample()`` end to end beside DPM-Solver++ at 20 steps.  TIME ONLY: the networks are untrained.
  ``--bench FILE ...``: files holding bench.py's JSON result line on this tree, copied into the record.

Usage:  python tools/edm_bench.py [--bench FILE ...]
"""
import argparse
import json
import os
import statistics
import sys
import time


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


def _bench_line(path):
    for ln in reversed(open(path).read().splitlines()):
        if ln.startswith("{"):
            r = json.loads(ln)
            keep = ("metric", "value", "unit", "images_per_sec", "step_ms", "ms_per_step", "mode")
            return {k: r[k] for k in keep if k in r} or r
    raise SystemExit(f"{path} holds no JSON result line")


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r21_edm_bench.json"))
    ap.add_argument("--bench", default=None, nargs="*")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    a = ap.parse_args()
    for p in (here, os.path.join(here, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import edm as plan
    from lgm_hip import ops
    from lgm_hip.graph import DDPMFastStep
    from models.generative.diffusion import ddpm as D
    from models.generative.diffusion import edm as E
    assert torch.cuda.is_available(), "edm_bench needs a GPU: it does not fall back"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)

    def module(cls, size, **kw):
        torch.manual_seed(0)
        m = cls(img_channels=3, img_size=size, dim=64, lr=8e-5, **kw)
        m.sample_every = 0
        m.to(dev)
        m.prepare_hip(dev)
        m.train()
        return m, m.configure_optimizers()

    def timed(variants, window=a.window, runs=a.runs):
        for run in variants.values():
            run(3)
        wall = {k: [] for k in variants}
        for _ in range(runs):
            for k, run in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(window)
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3 / window)
        return {k: round(statistics.median(v), 4) for k, v in wall.items()}

    out = {"what": f"UNet dim 64, one GPU, graph replay; ms: wall time of windows of {a.window} (torch.cuda.synchronize on both "
                   f"sides), median of {a.runs} windows after warm-up, the variants of one process alternating; us figures: 200 "
                   "back-to-back calls between two device events",
           "device": torch.cuda.get_device_name(0)}
    # ---- (i) the training step at 32 x 32, B = 128
    B, S, C = 128, 32, 3
    x = torch.rand(B, C, S, S, generator=g).to(dev)
    steps = {"ddpm": DDPMFastStep(*module(D.DDPM, S), 1, use_graph=True), "edm (learned frequencies)": module(E.EDM, S),
             "edm (random features)": module(E.EDM, S, random_fourier_features=True, learned_sinusoidal_cond=False)}
    for k in list(steps)[1:]:
        steps[k] = steps[k][0].make_fast_step(steps[k][1], 1, True)

    def fast_steps(fast):
        def run(n):
            for i in range(n):
                fast.step((x, None), i)
        return run
    ms = timed({k: fast_steps(f) for k, f in steps.items()})
    for k, f in steps.items():
        assert f.mode.startswith("hipGraph"), f"{k}: graph replay is unavailable"
    out["step_32_B128_ms"] = ms
    out["step_32_B128_edm_over_ddpm"] = round(ms["edm (learned frequencies)"] / ms["ddpm"], 4)
    out["step_32_B128_time_embedding_and_qsample_added_ms"] = round(ms["edm (learned frequencies)"] - ms["ddpm"], 4)
    out["notes"] = ("step_32_B128_time_embedding_and_qsample_added_ms is ONE figure: the Fourier network's unfused time-embedding "
                    "path and the other q_sample launch are not separated.  The us figures are back-to-back launches issued from "
                    "Python through ctypes: at 5 - 16 us they are bound by launch overhead and are an upper bound of the kernels' "
                    "own time, not a bandwidth measurement.")
    ed = steps["edm (learned frequencies)"].model.ema.online_model
    gd = steps["ddpm"].model.ema.online_model
    net = ed.model
    del steps

    # ---- (iii) the kernels alone
    noise = torch.randn(B, C, S, S, generator=g).to(dev)
    n = torch.randn(B, generator=g).to(dev)
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    q = E.edm_loss_qsample(ed, x, noise, True, n=n)
    sig, cn = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    st = E._State(net, (B, C, S, S), dev)
    st.x.normal_()
    F = torch.randn(B, S, S, 4, device=dev)
    row = plan.edm_plan(8, sigma_min=0.002, sigma_max=80.0, sigma_data=0.5, rho=7.0, S_churn=2.0)[3]
    L, s_ = ops.lib(), ops.stream()
    qd = D.hip_loss_qsample(gd, x, t, noise, True)

    def qsample():
        L.lgm_qsample_target_slice(x.data_ptr(), noise.data_ptr(), None, 0.0, t.data_ptr(), gd.sqrt_alphas_cumprod.data_ptr(),
                                   gd.sqrt_one_minus_alphas_cumprod.data_ptr(), 1, 2, qd.xt.data_ptr(), 4, 0, -1,
                                   qd.target.data_ptr(), 4, B, C, S * S, 4, s_)
    half, pe, gpe = net.fourier_half, torch.zeros(B, 20, device=dev), torch.randn(B, 20, device=dev)
    w = net.time_mlp[0].weights
    gw = torch.zeros(8, device=dev)
    px = B * S * S * 4 * 4
    img_b = 4 * B * C * S * S
    fns = {"qsample_target_slice": qsample,
           "edm_qsample": lambda: ops.edm_qsample(x, noise, q.xt, 0, q.target, sig, cn, 0.5, True, n=n, P_mean=-1.2, P_std=1.2),
           "edm_pre (with noise)": lambda: ops.edm_pre(st.x, noise, st.xhat, st.xin, 0, st.cnoise, C, row=row),
           "edm_euler (second evaluation follows)": lambda: ops.edm_euler(F, st.xhat, st.x, C, True, d=st.d, xin=st.xin,
                                                                          cnoise=st.cnoise, second=True, row=row),
           "edm_heun": lambda: ops.edm_heun(F, st.xhat, st.d, st.x, C, True, row=row),
           "fourier_emb_fwd": lambda: ops.fourier_emb_fwd(cn, net._flat.ptr(w), half, pe),
           "fourier_emb_bwd": lambda: ops.fourier_emb_bwd(pe, gpe, half, gw.data_ptr(), 0.0)}
    bytes_ = {"qsample_target_slice": 2 * img_b + 2 * px, "edm_qsample": 2 * img_b + 2 * px, "edm_pre (with noise)": img_b + 3 * px,
              "edm_euler (second evaluation follows)": 5 * px, "edm_heun": 5 * px}
    us = {k: alone(torch, f) for k, f in fns.items()}
    out["kernels_alone_B128_3x32x32"] = {"us": us, "algorithmic_bytes": bytes_,
                                         "TB_per_s": {k: round(bytes_[k] / us[k] * 1e-6, 3) for k in bytes_}}

    # ---- (ii), (iv) chains of 64 images at 64 x 64: time only
    Bs = 64
    unet_d, unet_e = D.Unet(dim=64), D.Unet(dim=64, learned_sinusoidal_cond=True)
    chains = {"ddim 32": D.GaussianDiffusion(unet_d, img_size=64, sampling_timesteps=32).to(dev),
              "dpm++ 20": D.GaussianDiffusion(unet_d, img_size=64, sampling_timesteps=20, sampler="dpm++").to(dev),
              "edm heun 32": E.ElucidatedDiffusion(unet_e, img_size=64, num_sample_steps=32).to(dev),
              "edm euler 32": E.ElucidatedDiffusion(unet_e, img_size=64, num_sample_steps=32, sampler="euler").to(dev)}
    unet_d.prepare_hip(dev)
    unet_e.prepare_hip(dev)
    with torch.no_grad():
        res = timed({k: (lambda n_, c=c: [c.sample(batch_size=Bs) for _ in range(n_)]) for k, c in chains.items()}, window=1,
                    runs=5)
    out["sample_64_at_64x64_ms (time only: untrained networks, sample quality is not measured)"] = res
    out["per_step_ms_64_at_64x64"] = {"ddim step": round(res["ddim 32"] / 32, 4), "two ddim steps": round(res["ddim 32"] / 16, 4),
                                      "euler step": round(res["edm euler 32"] / 32, 4),
                                      "heun step (31 with two forwards, 1 with one)": round(res["edm heun 32"] / 32, 4)}
    if a.bench:
        out["bench_py"] = [_bench_line(f) for f in a.bench]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
