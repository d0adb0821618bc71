"""Generate tests/golden/nice.npz: the REAL reference's ``NICE`` (models/generative/flow/nice.py) on the CPU in float32, one
``training_step`` and its backward and one ``forward(z, reverse=True)``, for two cases (the reference fixes hidden_dim = 256
and 4 coupling layers):
a  input_dim = 20, B = 5: halves of 10 lanes start 8-byte aligned but not 16-byte aligned;  b  input_dim = 6, B = 3: halves
of 3 lanes.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_dae.py, whose stubs (oracle.make_golden.install_stubs) and ``--check`` mode
it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_nice.py [--check]

Recipe: weights ``tests/nice_ref.nice_init(D, 4, 256, seed)`` (log_scale about 0.3 randn, so the scaling layer takes part); x
uniform in (-1, 1) from ``torch.Generator().manual_seed(seed + 1)``.  Stored per case: x, z, the loss, every parameter
gradient, ``forward(z, reverse=True)`` and the seed.
LeakyReLU has a kink: a float32 run on the other side of it differs from the float64 model by a slope.  The tool therefore walks
the seed upwards from the case's first one until (a) every hidden pre-activation of the float64 forward is >= 1e-5 from zero
and (b) that smallest distance from zero is >= 10 times the largest float32-to-float64 distance of those inputs, which it
measures itself; the seed and both figures are stored.
The tool also asserts once, in float64 at D = 6, the sign of the change of variables: log N(z; 0, I) + log |det dz/dx| with
the Jacobian from ``torch.autograd.functional.jacobian`` equals -0.5 sum z^2 - 0.5 D log 2 pi + sum log_scale to 1e-10, and the
reference's own ``_compute_loss`` misses the mean of it by 2 sum log_scale."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "nice.npz")

LAYERS, HIDDEN = 4, 256
CASES = {"a": (20, 5, 0), "b": (6, 3, 10)}     # (input_dim, B, first seed)
MARGIN = 1e-5


def case_x(D, B, seed):
    return torch.rand(B, D, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1


def const_shift(D):
    """The reference forms 0.5 D log 2 pi from a float32 tensor, in a float64 model too: what that adds to its log-likelihood"""
    import nice_ref as NR
    return -(float(0.5 * D * torch.log(2 * torch.tensor(torch.pi))) - 0.5 * D * NR.LOG_2PI)


def check_change_of_variables(R, NR):
    """float64, D = 6: the density's log-determinant enters with a plus sign"""
    D, B = 6, 3
    P = {k: v.double() for k, v in NR.nice_init(D, LAYERS, HIDDEN, 99).items()}
    net = R.NICE(D, LAYERS).double()
    net.load_state_dict(P, strict=True)
    x = case_x(D, B, 99).double()
    o, _ = NR.forward(P, x)
    worst = 0.0
    for b in range(B):
        J = torch.autograd.functional.jacobian(lambda v: net(v[None])[0], x[b])
        z = net(x[b][None])[0].detach()
        want = -0.5 * (z ** 2).sum() - 0.5 * D * NR.LOG_2PI + torch.linalg.slogdet(J)[1]
        worst = max(worst, abs(float(want - o["log_prob"][b])))
    assert worst < 1e-10, worst
    ref = net._compute_loss(net(x), x).detach()                      # what the reference calls the mean log-likelihood
    gap = float(o["log_prob"].mean() - ref) + const_shift(D)
    assert abs(gap - 2 * float(o["sum_ls"])) < 1e-10 and abs(gap) > 1e-3, gap
    print(f"change of variables at D = 6: log_prob against the Jacobian {worst:.1e}; the reference's sign misses the mean by "
          f"2 sum log_scale = {gap:.6f}")


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.flow import nice as R
    import nice_ref as NR

    torch.set_num_threads(8)
    check_change_of_variables(R, NR)
    fx = {"margin": MARGIN, "cases": np.asarray(sorted(CASES)), "keys": np.asarray(NR.keys(LAYERS)),
          "layers": LAYERS, "hidden": HIDDEN}
    for name, (D, B, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 50):
            P = NR.nice_init(D, LAYERS, HIDDEN, seed)
            x = case_x(D, B, seed)
            P64 = {k: v.double() for k, v in P.items()}
            o64, t64 = NR.forward(P64, x.double())
            _, t32 = NR.forward(P, x)
            margin = NR.kink_margin(t64)
            dist = float((NR.kink_values(t32).double() - NR.kink_values(t64)).abs().max())
            if margin >= MARGIN and margin >= 10 * dist:
                break
        else:
            raise SystemExit(f"case {name}: no seed in 50 holds the margins")
        print(f"case {name}: seed {seed}, kink margin {margin:.3e}, float32 distance {dist:.3e}")

        def network(double=False):
            net = R.NICE(D, LAYERS)
            net.load_state_dict(P, strict=True)
            net.train()
            net.log = lambda *a, **k: None
            return net.double() if double else net

        net = network()
        assert list(net.state_dict().keys()) == NR.keys(LAYERS) == [n for n, _ in net.named_parameters()]
        z = net(x).detach()
        loss = net.training_step((x, torch.zeros(B, dtype=torch.long)), 0)
        loss.backward()
        x_back = net(z, reverse=True).detach()
        n64 = network(True)
        loss64 = n64.training_step((x.double(), None), 0)
        loss64.backward()
        # the restatement is the reference
        assert float((o64["z"] - n64(x.double()).detach()).abs().max()) < 1e-12
        assert abs(float(o64["loss"] - loss64.detach()) - const_shift(D)) < 1e-12
        G64 = NR.backward(P64, t64)
        for n, p in n64.named_parameters():
            assert float((G64[n] - p.grad).abs().max()) < 1e-12, n
        assert float((NR.inverse(P64, o64["z"]) - x.double()).abs().max()) < 1e-12
        pre = f"{name}:"
        fx.update({pre + "dims": np.asarray([D, B]), pre + "seed": seed, pre + "kink_margin": margin, pre + "f32_distance": dist,
                   pre + "x": x.numpy(), pre + "z": z.numpy(), pre + "loss": loss.detach().numpy(), pre + "inverse": x_back.numpy()})
        worst = 0.0
        for (n, p), (_, p64) in zip(net.named_parameters(), n64.named_parameters()):
            worst = max(worst, float((p.grad.double() - p64.grad).norm() / p64.grad.norm()))
            fx[f"{pre}shape:{n}"] = np.asarray(p.shape)
            fx[f"{pre}grad:{n}"] = p.grad.reshape(-1).numpy().copy()
        fx[pre + "f32_grad_distance"] = worst
        fx[pre + "f32_roundtrip"] = float((x_back - x).abs().max())
        print(f"case {name}: loss {float(loss.detach()):.6f} (float64 {float(loss64.detach()):.6f}), worst float32-to-float64 "
              f"gradient distance {worst:.2e} relative, round trip {float((x_back - x).abs().max()):.1e}")
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
