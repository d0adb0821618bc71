"""Measure the MLP GAN on the HIP path -> profiles/r24_gan_bench.json.  Needs a GPU; nothing falls back.

  (i)   alone, between device events, median of ``--runs`` alternating windows of ``--window`` calls: ``lgm_bn1d_fwd`` /
        ``lgm_bn1d_bwd`` beside the existing two-launch pairs (``lgm_bn_stats`` + ``lgm_bn_affine3``; the LeakyReLU
        derivative, ``lgm_bn_reduce3_coef`` + ``lgm_bn_affine3``) on the SAME operands through ``BatchNorm1d.fwd`` / ``bwd``
        under both routes, at B = 32 and 256 and F = 256, 512, 1024 - this decides ``BatchNorm1d.route``; the BCE kernels
        beside the ATen sequence ``DCGAN`` uses on [B] logits (forward, and forward + backward);
  (ii)  the training step of configs/gan/gan.json at B = 32 (the config) and B = 256: graph replay, the same step object
        issuing eager launches, and the same module's plain-torch layers (``G.model`` / ``D.model``, autograd,
        ``torch.optim.Adam``) on the same device - the comparator: there is no parent-commit step, the model did not exist;
  (iii) with ``--parent DIR`` (a checkout of the parent commit, its library built): ``bench.py`` (DDPM 32 x 32 and
        ``--workload vqvae``) on this tree and on the parent's, alternating, ``--bench-rounds`` times each.
TIME ONLY: the networks are untrained.

Usage:  python tools/gan_bench.py [--parent DIR] [--bench-rounds N]
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


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r24_gan_bench.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (bench.py needs its library built)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window", type=int, default=20)
    a = ap.parse_args()
    for p in (here, os.path.join(here, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import ops
    from lgm_hip.bn import BatchNorm1d
    from lgm_hip.flat import FlatParams
    from lgm_hip.lightning import _CountingOptimizer
    from lgm_hip.nn import GradCtx, param_kind
    from utils.loader import load_config, load_model
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    default_route = BatchNorm1d.route
    rec = {"runs": a.runs, "window": a.window, "unit": "us per call, median of alternating windows", "kernels": {},
           "default_route": default_route}
    cfg = load_config(os.path.join(here, "lightning-generative-models_amd", "configs", "gan", "gan.json"))

    # (i) kernels
    for B in (32, 256):
        for F in (256, 512, 1024):
            gen = torch.Generator().manual_seed(B + F)
            bn = BatchNorm1d(F).to(dev)
            flat = FlatParams([(n, p, param_kind(n, p)) for n, p in bn.named_parameters()], dev)
            act_in, gy = (torch.randn(B, F, generator=gen) + 3).to(dev), torch.randn(B, F, generator=gen).to(dev)
            saved = {}
            for route in ("rows", "generic"):
                BatchNorm1d.route = route
                saved[route] = bn.fwd(act_in, ops.ACT_LRELU, 0.2, True)

            def fwd(route):
                def f():
                    BatchNorm1d.route = route
                    bn.fwd(act_in, ops.ACT_LRELU, 0.2, True)
                return f

            def bwd(route):
                y, sv = saved[route]

                def f():
                    flat.zero_grad()
                    bn.bwd(GradCtx(flat, transposed=False), sv, y, gy, ops.ACT_LRELU, 0.2)
                return f
            for name, mk in (("bn_fwd", fwd), ("bn_bwd", bwd)):
                t = alternate(torch, {r: mk(r) for r in ("rows", "generic")}, a.runs, a.window)
                t["rows_over_generic"] = round(t["rows"] / t["generic"], 3)
                rec["kernels"][f"{name} B{B} F{F}"] = t
                print(f"{name} B{B} F{F}: {t}", flush=True)
            BatchNorm1d.route = default_route
            rec["kernels"][f"bn_fwd B{B} F{F}"]["rel_diff_rows_vs_generic"] = float(
                (saved["rows"][0] - saved["generic"][0]).norm() / saved["generic"][0].norm())
        # the loss head alone, beside the ATen sequence on [B] logits
        gen = torch.Generator().manual_seed(B)
        s_r, s_f = torch.randn(B, 4, generator=gen).to(dev), torch.randn(B, 4, generator=gen).to(dev)
        vals5, vals2, gl = torch.empty(5, device=dev), torch.empty(2, device=dev), torch.ones(1, device=dev)
        g_r, g_f = torch.empty(B, 4, device=dev), torch.empty(B, 4, device=dev)
        lr, lf = s_r[:, 0].clone().requires_grad_(), s_f[:, 0].clone().requires_grad_()
        bce = torch.nn.functional.binary_cross_entropy_with_logits

        def aten_d(backward):
            def f():
                real, fake = bce(lr, torch.ones_like(lr)), bce(lf, torch.zeros_like(lf))
                d = (real + fake) / 2
                lr.mean(), lf.mean()
                if backward:
                    lr.grad = lf.grad = None
                    d.backward()
            return f
        t = alternate(torch, {
            "gan_bce_d": lambda: ops.gan_bce_d(s_r, s_f, vals5),
            "aten_d_fwd": aten_d(False),
            "gan_bce_d+bwd": lambda: (ops.gan_bce_d(s_r, s_f, vals5), ops.gan_bce_bwd(gl, s_r, 1.0, 0.5, g_r, s_f, 0.0, 0.5, g_f)),
            "aten_d_fwd+bwd": aten_d(True),
            "gan_bce_g": lambda: ops.gan_bce_g(s_f, "non-saturating", vals2),
            "gan_bce_g+bwd": lambda: (ops.gan_bce_g(s_f, "non-saturating", vals2), ops.gan_bce_bwd(gl, s_f, 1.0, 1.0, g_f))},
            a.runs, a.window)
        rec["kernels"][f"loss head B{B}"] = t
        print(f"loss head B{B}: {t}", flush=True)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    save()

    # (ii) the training step
    rec["train_step"] = {}
    for B in (32, 256):
        img = torch.rand(B, 1, 28, 28, device=dev) * 2 - 1
        batch = (img, None)
        fns, keep = {}, []
        for name, graph in (("replay", True), ("eager_launches", False)):
            torch.manual_seed(0)
            m = load_model(cfg["model"]).to(dev)
            m.prepare_hip(dev)
            m.train()
            m._optimizers = [_CountingOptimizer(o, m) for o in m.configure_optimizers()[0]]
            fast = m.make_fast_step(m._optimizers, 1, graph)
            for i in range(3):
                fast.step(batch, i)
            keep.append((m, fast))
            fns[name] = (lambda f: lambda: f.step(batch, 0))(fast)
        modes = {"replay": keep[0][1].mode, "eager_launches": keep[1][1].mode, "bn_route": default_route}
        # the same module's plain-torch layers on the device (no flat storage: G.model / D.model are ordinary torch modules)
        torch.manual_seed(0)
        pm = load_model(cfg["model"]).to(dev)
        pm.train()
        hp = pm.hparams
        kw = dict(lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)
        d_opt, g_opt = torch.optim.Adam(pm.D.parameters(), **kw), torch.optim.Adam(pm.G.parameters(), **kw)
        L = hp.latent_dim

        def plain_step():
            x_hat = pm.G.model(torch.randn([B, L], device=dev))
            s_r, s_f = pm.D.model(img.view(B, -1)).squeeze(), pm.D.model(x_hat.detach()).squeeze()
            d_loss = (bce(s_r, torch.ones_like(s_r)) + bce(s_f, torch.zeros_like(s_f))) / 2
            s_r.mean(), s_f.mean()
            d_opt.zero_grad(set_to_none=True)
            d_loss.backward()
            d_opt.step()
            s = pm.D.model(x_hat).squeeze()
            g_loss = bce(s, torch.ones_like(s))
            s.mean()
            g_opt.zero_grad(set_to_none=True)
            g_loss.backward()
            g_opt.step()
        fns["plain_torch"] = plain_step
        modes["plain_torch"] = "the module's torch layers, autograd, torch.optim.Adam, same device"
        t = alternate(torch, fns, a.runs, a.window)
        t["modes"] = modes
        t["plain_over_replay"] = round(t["plain_torch"] / t["replay"], 2)
        rec["train_step"][f"B{B}"] = t
        print(f"train step B{B}: {t}", flush=True)
        del keep, fns
    save()

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
    save()
    print(a.out)


if __name__ == "__main__":
    main()
