"""Generate tests/golden/vae.npz: the REAL reference's ``VAE`` (models/generative/vae/vae.py) on the CPU in float32, one
training-mode ``_common_step`` and its backward, for two small cases (C, S, L, B) = (1, 8, 4, 4) and (3, 5, 3, 3).

TEST INFRASTRUCTURE ONLY, like tools/make_golden_pixelcnn.py, whose stubs (oracle.make_golden.install_stubs) and ``--check``
mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_vae.py [--check]

Recipe: weights ``tests/vae_ref.vae_init(C, S, L, seed)``; x uniform in (-1, 1) and eps normal from
``torch.Generator().manual_seed(seed + 1)``; eps is injected by patching ``torch.randn_like``.  Stored per case: x, eps, mu,
log_var, x_hat, the three losses and every parameter gradient (whole up to 4096 elements, else its float64 norm + a
1024-element strided sample).
LeakyReLU and |.| have kinks: a float32 run on the other side of one differs from the float64 model by a whole slope.  The
tool therefore walks the seed upwards from the case's first one until (a) every LeakyReLU input and every x_hat - x of the
float64 forward is >= 1e-5 from zero and (b) 1e-5 is >= 10 times the largest float32-to-float64 distance of those
quantities, which it measures itself; the seed and both figures are stored."""
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
OUT = os.path.join(ROOT, "tests", "golden", "vae.npz")

CASES = {"a": (1, 8, 4, 4, 2301), "b": (3, 5, 3, 3, 2311)}          # (C, S, L, B, first seed)
KLD_WEIGHT = 1e-2
MARGIN = 1e-5
WHOLE, SAMPLE = 4096, 1024


def case_data(C, S, B, L, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.rand(B, C, S, S, generator=g) * 2 - 1, torch.randn(B, L, generator=g)


def kink_values(tape):
    x2, _, _, epres, _, dpres, o = tape
    return torch.cat([p.reshape(-1) for p in epres] + [p.reshape(-1) for p in dpres[:3]] + [(o["x_hat"] - x2).reshape(-1)])


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    try:
        import pandas  # noqa: F401
    except ImportError:
        sys.modules["pandas"] = types.ModuleType("pandas")
    from models.generative.vae import vae as R
    import vae_ref as VR

    torch.set_num_threads(8)
    fx = {"kld_weight": KLD_WEIGHT, "margin": MARGIN, "grad_sample": SAMPLE, "cases": np.asarray(sorted(CASES))}
    for name, (C, S, L, B, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 50):
            P = VR.vae_init(C, S, L, seed)
            x, eps = case_data(C, S, B, L, seed)
            P64 = {k: v.double() for k, v in P.items()}
            o64, t64 = VR.forward(P64, x.double(), eps.double(), KLD_WEIGHT)
            _, t32 = VR.forward(P, x, eps, KLD_WEIGHT)
            margin = VR.kink_margin(t64)
            dist = float((kink_values(t32).double() - kink_values(t64)).abs().max())
            if margin >= MARGIN and MARGIN >= 10 * dist:
                break
        else:
            raise SystemExit(f"case {name}: no seed in 50 holds the margins")
        print(f"case {name}: seed {seed}, kink margin {margin:.3e}, float32 distance {dist:.3e}")

        def network(double=False):
            net = R.VAE(C, S, latent_dim=L, kld_weight=KLD_WEIGHT)
            net.load_state_dict(P, strict=True)
            net.train()
            return net.double() if double else net

        real_randn_like = torch.randn_like
        try:
            torch.randn_like = lambda t, *a, **k: eps.to(t.dtype)
            net = network()
            assert list(net.state_dict().keys()) == VR.KEYS
            x_hat, mu, lv = net(x)
            loss = net._common_step((x, torch.zeros(B, dtype=torch.long)), 0, "train")
            loss.backward()
            n64 = network(True)
            xh64, mu64, lv64 = n64(x.double())
            loss64 = n64._common_step((x.double(), torch.zeros(B, dtype=torch.long)), 0, "train")
            loss64.backward()
        finally:
            torch.randn_like = real_randn_like
        # the restatement is the reference
        assert float((o64["x_hat"].view_as(xh64) - xh64.detach()).abs().max()) < 1e-12
        assert abs(float(o64["loss"] - loss64.detach())) < 1e-12
        G64 = VR.backward(P64, t64, KLD_WEIGHT)
        worst = 0.0
        for n, p in n64.named_parameters():
            assert float((G64[n] - p.grad).abs().max()) < 1e-12, n
        recon = torch.nn.functional.l1_loss(x_hat, x)
        kld = -0.5 * torch.mean(1 + lv - mu.pow(2) - lv.exp())
        pre = f"{name}:"
        fx.update({pre + "dims": np.asarray([C, S, L, B]), pre + "seed": seed, pre + "kink_margin": margin,
                   pre + "f32_distance": dist, pre + "x": x.numpy(), pre + "eps": eps.numpy(),
                   pre + "mu": mu.detach().numpy(), pre + "log_var": lv.detach().numpy(),
                   pre + "x_hat": x_hat.detach().numpy(), pre + "loss": loss.detach().numpy(),
                   pre + "recon": recon.detach().numpy(), pre + "kld": kld.detach().numpy()})
        for (n, p), (_, p64) in zip(net.named_parameters(), n64.named_parameters()):
            flat = p.grad.reshape(-1)
            worst = max(worst, float((flat.double() - p64.grad.reshape(-1)).norm() / p64.grad.norm()))
            if flat.numel() <= WHOLE:
                fx[f"{pre}grad:{n}"] = flat.numpy().copy()
            else:
                fx[f"{pre}gradnorm:{n}"] = np.float64(flat.double().norm().item())
                fx[f"{pre}gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[pre + "f32_grad_distance"] = worst
        print(f"case {name}: loss {float(loss.detach()):.6f} (float64 {float(loss64):.6f}), worst float32-to-float64 "
              f"gradient distance {worst:.2e} relative")
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
