"""Generate tests/golden/dae.npz: the REAL reference's ``DAE`` (models/generative/autoencoder/dae.py) on the CPU in float32, one
training-mode ``_common_step`` and its backward, for two cases at 1 x 28 x 28 (the only size the reference accepts):
a  B = 4, gaussian, level 0.1;  b  B = 3, salt_and_pepper, level 0.2.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_vae.py, whose stubs (oracle.make_golden.install_stubs) and ``--check`` mode
it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_dae.py [--check]

Recipe: weights ``tests/dae_ref.dae_init(1, 28, seed)``; x uniform in (-1, 1), then the draws (one normal draw, or the salt
and the pepper uniform draws) from ``torch.Generator().manual_seed(seed + 1)``; the draws are injected by patching
``torch.randn_like`` / ``torch.rand_like`` (salt is drawn first).  Stored per case: x, the draws, the corrupted input, x_hat, the
loss and every parameter gradient (whole up to 4096 elements, else its float64 norm + a 1024-element strided sample).
ReLU has a kink: a float32 run on the other side of it differs from the float64 model by a whole slope.  The tool therefore
walks the seed upwards from the case's first one until (a) every ReLU input of the float64 forward is >= 1e-5 from zero and
(b) 1e-5 is >= 10 times the largest float32-to-float64 distance of those inputs, which it measures itself; the seed and both
figures are stored."""
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
OUT = os.path.join(ROOT, "tests", "golden", "dae.npz")

C, S = 1, 28
CASES = {"a": (4, "gaussian", 0.1, 2501), "b": (3, "salt_and_pepper", 0.2, 2511)}     # (B, noise_type, level, first seed)
MARGIN = 1e-5
WHOLE, SAMPLE = 4096, 1024


def case_data(B, noise_type, seed):
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(B, C, S, S, generator=g) * 2 - 1
    if noise_type == "gaussian":
        return x, torch.randn(B, C, S, S, generator=g)
    return x, torch.stack([torch.rand(B, C, S, S, generator=g), torch.rand(B, C, S, S, generator=g)])


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    try:
        import pandas  # noqa: F401
    except ImportError:
        sys.modules["pandas"] = types.ModuleType("pandas")
    from models.generative.autoencoder import dae as R
    import dae_ref as DR

    torch.set_num_threads(8)
    fx = {"margin": MARGIN, "grad_sample": SAMPLE, "cases": np.asarray(sorted(CASES)), "keys": np.asarray(DR.KEYS)}
    for name, (B, noise_type, level, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 50):
            P = DR.dae_init(C, S, seed)
            x, draws = case_data(B, noise_type, seed)
            P64 = {k: v.double() for k, v in P.items()}
            xc = DR.corrupt(x, noise_type, level, draws)     # float32, as the reference forms it
            o64, t64 = DR.forward(P64, x.double(), xc.double())
            _, t32 = DR.forward(P, x, xc)
            margin = DR.kink_margin(t64)
            dist = float((DR.kink_values(t32).double() - DR.kink_values(t64)).abs().max())
            if margin >= MARGIN and MARGIN >= 10 * dist:
                break
        else:
            raise SystemExit(f"case {name}: no seed in 50 holds the margins")
        print(f"case {name}: seed {seed}, kink margin {margin:.3e}, float32 distance {dist:.3e}")

        def network(double=False):
            net = R.DAE(C, S, noise_type=noise_type, noise_level=level)
            net.load_state_dict(P, strict=True)
            net.train()
            return net.double() if double else net

        real_randn_like, real_rand_like = torch.randn_like, torch.rand_like
        queue = []

        def fake_rand_like(t, *a, **k):
            return queue.pop(0).to(t.dtype)
        try:
            torch.randn_like = lambda t, *a, **k: draws.to(t.dtype)
            torch.rand_like = fake_rand_like
            net = network()
            assert list(net.state_dict().keys()) == DR.KEYS
            queue[:] = list(draws) if noise_type != "gaussian" else []
            noisy = net.add_noise(x)
            assert torch.equal(noisy, xc), "the restated corruption is the reference's, to the bit"
            x_hat = net(noisy)
            queue[:] = list(draws) if noise_type != "gaussian" else []
            loss = net._common_step((x, torch.zeros(B, dtype=torch.long)), 0)
            loss.backward()
            n64 = network(True)
            queue[:] = list(draws) if noise_type != "gaussian" else []
            # the float64 model of the SAME corrupted input (the float32 corruption, widened)
            xh64 = n64(xc.double())
            loss64 = n64.metric(x.double(), xh64)
            loss64.backward()
        finally:
            torch.randn_like, torch.rand_like = real_randn_like, real_rand_like
        # the restatement is the reference
        assert float((o64["x_hat"].view_as(xh64) - xh64.detach()).abs().max()) < 1e-12
        assert abs(float(o64["loss"] - loss64.detach())) < 1e-12
        G64 = DR.backward(P64, t64)
        worst = 0.0
        for n, p in n64.named_parameters():
            assert float((G64[n] - p.grad).abs().max()) < 1e-12, n
        pre = f"{name}:"
        fx.update({pre + "dims": np.asarray([C, S, B]), pre + "seed": seed, pre + "noise_type": noise_type, pre + "level": level,
                   pre + "kink_margin": margin, pre + "f32_distance": dist, pre + "x": x.numpy(), pre + "draws": draws.numpy(),
                   pre + "corrupted": noisy.numpy(), pre + "x_hat": x_hat.detach().numpy(), pre + "loss": loss.detach().numpy()})
        for (n, p), (_, p64) in zip(net.named_parameters(), n64.named_parameters()):
            flat = p.grad.reshape(-1)
            worst = max(worst, float((flat.double() - p64.grad.reshape(-1)).norm() / p64.grad.norm()))
            fx[f"{pre}shape:{n}"] = np.asarray(p.shape)
            if flat.numel() <= WHOLE:
                fx[f"{pre}grad:{n}"] = flat.numpy().copy()
            else:
                fx[f"{pre}gradnorm:{n}"] = np.float64(flat.double().norm().item())
                fx[f"{pre}gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[pre + "f32_grad_distance"] = worst
        print(f"case {name}: loss {float(loss.detach()):.6f} (float64 {float(loss64.detach()):.6f}), worst float32-to-float64 "
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
