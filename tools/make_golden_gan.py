"""Generate tests/golden/gan_mlp.npz: the REAL reference's ``GAN`` (models/generative/gan/gan.py) on the CPU in float32 - one
training-mode generator forward with z injected, the discriminator loss with its backward, and the generator loss with its
backward for both loss types - for two small cases (C, S, L, B) = (1, 8, 6, 5) and (3, 5, 3, 4); the hidden widths are the
reference's.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_vae.py, whose stubs (oracle.make_golden.install_stubs) and ``--check`` mode it
shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_gan.py [--check]

Recipe: weights ``tests/gan_ref.gan_init(C, S, L, seed)``; x uniform in (-1, 1) and z normal from
``torch.Generator().manual_seed(seed + 1)``; z is handed to the reference's ``Generator.forward``.  Stored per case: z, x,
x_hat, the logits, every loss, the running statistics after the forward and every gradient (whole up to 4096 elements, else
its float64 norm + a 1024-element strided sample).
LeakyReLU has a kink: a float32 run on the other side of it differs from the float64 model by a whole slope.  The tool
therefore walks the seed upwards from the case's first one until (a) every LeakyReLU input of the float64 forwards (G on z, D
on x and on G(z)) is >= 1e-5 from zero and (b) that margin is >= 10 times the largest float32-to-float64 distance of those
inputs, which it measures itself; the seed and both figures are stored."""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "gan_mlp.npz")

CASES = {"a": (1, 8, 6, 5, 2401), "b": (3, 5, 3, 4, 2411)}          # (C, S, L, B, first seed)
MARGIN = 1e-5
WHOLE, SAMPLE = 4096, 1024


def case_data(C, S, B, L, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.rand(B, C, S, S, generator=g) * 2 - 1, torch.randn(B, L, generator=g)


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    try:
        import pandas  # noqa: F401
    except ImportError:
        sys.modules["pandas"] = types.ModuleType("pandas")
    from models.generative.gan import gan as R
    import gan_ref as GR

    torch.set_num_threads(8)
    fx = {"margin": MARGIN, "grad_sample": SAMPLE, "cases": np.asarray(sorted(CASES)),
          "loss_types": np.asarray(GR.LOSS_TYPES)}
    for name, (C, S, L, B, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 50):
            P = GR.gan_init(C, S, L, seed)
            x, z = case_data(C, S, B, L, seed)
            P64 = GR.to64(P)
            k64 = GR.kink_values(P64, z.double(), x.double())
            margin = float(k64.abs().min())
            dist = float((GR.kink_values(P, z, x).double() - k64).abs().max())
            if margin >= MARGIN and margin >= 10 * dist:
                break
        else:
            raise SystemExit(f"case {name}: no seed in 50 holds the margins")
        print(f"case {name}: seed {seed}, kink margin {margin:.3e}, float32 distance {dist:.3e}")

        def run(double: bool):
            """the reference's module: one G forward, the D loss and both G losses with their backwards"""
            net = R.GAN(img_channels=C, img_size=S, latent_dim=L, summary=False)
            net.load_state_dict(P, strict=True)
            net.train()
            xx, zz = x, z
            if double:
                net, xx, zz = net.double(), x.double(), z.double()
            assert list(net.state_dict().keys()) == GR.KEYS
            out = {}
            x_hat = net.G(zz)
            d = net._calculate_d_loss(xx, x_hat)
            d["d_loss"].backward()
            out.update({k: v.detach() for k, v in d.items()})
            out["x_hat"] = x_hat.detach()
            out["s_real"], out["s_fake"] = net.D(xx).detach(), net.D(x_hat.detach()).detach()
            out["grad:D"] = {n: p.grad.clone() for n, p in net.D.named_parameters()}
            out["running"] = {k: v.detach().clone() for k, v in net.G.state_dict().items() if "running" in k}
            out["nbt"] = [int(v) for k, v in net.G.state_dict().items() if k.endswith("num_batches_tracked")]
            for lt in GR.LOSS_TYPES:
                net.hparams.loss_type = lt
                net.zero_grad(set_to_none=True)
                g = net._calculate_g_loss(x_hat)
                g["g_loss"].backward(retain_graph=True)
                out[f"g_loss:{lt}"] = g["g_loss"].detach()
                out[f"grad:G:{lt}"] = {n: p.grad.clone() for n, p in net.G.named_parameters()}
            return out

        o32, o64 = run(False), run(True)
        # the restatement is the reference
        xh64, tape, running = GR.g_forward(P64, z.double(), True)
        assert float((xh64 - o64["x_hat"].reshape(B, -1)).abs().max()) < 1e-12
        d64, GD = GR.d_loss(P64, x.double(), xh64)
        for k in ("d_loss", "d_loss_real", "d_loss_fake", "logits_real", "logits_fake"):
            assert abs(float(d64[k] - o64[k])) < 1e-12, k
        for n, g in GD.items():
            assert float((g - o64["grad:D"][n]).abs().max()) < 1e-12, n
        for k, v in running.items():
            assert float((v - o64["running"][k[2:]]).abs().max()) < 1e-12, k
        assert o64["nbt"] == [1, 1, 1]
        for lt in GR.LOSS_TYPES:
            loss, _, _, gxh = GR.g_loss(P64, xh64, lt)
            assert abs(float(loss - o64[f"g_loss:{lt}"])) < 1e-12
            for n, g in GR.g_backward(P64, tape, gxh).items():
                ref = o64[f"grad:G:{lt}"][n]
                assert float((g - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max())), (lt, n)

        pre = f"{name}:"
        fx.update({pre + "dims": np.asarray([C, S, L, B]), pre + "seed": seed, pre + "kink_margin": margin,
                   pre + "f32_distance": dist, pre + "x": x.numpy(), pre + "z": z.numpy(),
                   pre + "x_hat": o32["x_hat"].numpy(), pre + "s_real": o32["s_real"].numpy(),
                   pre + "s_fake": o32["s_fake"].numpy()})
        for k in ("d_loss", "d_loss_real", "d_loss_fake", "logits_real", "logits_fake"):
            fx[pre + k] = o32[k].numpy()
        for lt in GR.LOSS_TYPES:
            fx[f"{pre}g_loss:{lt}"] = o32[f"g_loss:{lt}"].numpy()
        for k, v in o32["running"].items():
            fx[f"{pre}G.{k}"] = v.numpy()
        worst = 0.0
        grads = [(f"D.{n}", g, o64["grad:D"][n]) for n, g in o32["grad:D"].items()]
        for lt in GR.LOSS_TYPES:
            grads += [(f"G:{lt}:{n}", g, o64[f"grad:G:{lt}"][n]) for n, g in o32[f"grad:G:{lt}"].items()]
        for n, g, g64 in grads:
            flat = g.reshape(-1)
            if not n.endswith((".0.bias", ".3.bias", ".6.bias")) or n.startswith("D."):
                worst = max(worst, float((flat.double() - g64.reshape(-1)).norm() / g64.norm()))
            if flat.numel() <= WHOLE:
                fx[f"{pre}grad:{n}"] = flat.numpy().copy()
            else:
                fx[f"{pre}gradnorm:{n}"] = np.float64(flat.double().norm().item())
                fx[f"{pre}gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[pre + "f32_grad_distance"] = worst
        print(f"case {name}: d_loss {float(o32['d_loss']):.6f} (float64 {float(o64['d_loss']):.6f}), worst float32-to-float64 "
              f"gradient distance {worst:.2e} relative (the analytically zero biases in front of a BatchNorm left out)")
    return {k: np.asarray(v) for k, v in fx.items()}


if __name__ == "__main__":
    fx = generate()
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as d:
            np.savez_compressed(os.path.join(d, "again.npz"), **fx)
            same = open(os.path.join(d, "again.npz"), "rb").read() == open(OUT, "rb").read()
        print(f"{OUT}: {'identical' if same else 'DIFFERS'}")
        sys.exit(0 if same else 1)
    np.savez_compressed(OUT, **fx)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
