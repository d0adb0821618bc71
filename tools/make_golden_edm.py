"""Generate tests/golden/diffusion_edm.npz: elucidated diffusion (Karras et al. 2022) around the REAL reference's
``Unet(learned_sinusoidal_cond=True)`` / ``Unet(random_fourier_features=True)`` on CPU, in float32 and float64, with the
textbook formulas written out here: the denoiser D = c_skip x + c_out F(c_in x, ln(sigma) / 4), the loss
mean_b mean_elem lambda(sigma_b) (D - y)^2 with ALL parameter gradients by autograd, and chains of Algorithm 2.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_distill.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_edm.py [--check]

Recipe: the small UNet of diffusion_unet_small.npz (dim 16, 16 x 16, B = 4, data seed 101), weights oracle.unet_init(seed=3)
for every tensor it knows; the tensors it does not know are drawn from seed 2101 and stored whole: ``time_mlp.0.weights`` [8]
(N(0, 1)), ``time_mlp.1.weight`` [64, 17] / ``.bias`` [64] (uniform at the fan-in bound) and ``label_emb.weight`` [4, 64]
(N(0, 1); K = 3 classes and the null label) for the guided chain.  sigma = (0.002, 0.5, 80, 1.7) for the loss.
Stored: the reference's state-dict keys and shapes (learned and random), F in float32 and float64, the loss in both, every
gradient (whole up to 512 elements, else norm + a 128-element strided sample), and per chain the start, the injected noises,
the final image in float32 and float64 and their distance relative to max |image|.  The tool asserts that the churned chain
has gamma > 0 on at least half its steps and that the clamp changes D in at least one step of every chain."""
from __future__ import annotations

import math
import os
import sys
import tempfile

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_edm.npz")

WHOLE, SAMPLE = 512, 128
SEED, EXTRA_SEED, K = 3, 2101, 3
SIGMAS = (0.002, 0.5, 80.0, 1.7)
SD, SMIN, SMAX, RHO, S_TMIN, S_TMAX, S_NOISE = 0.5, 0.002, 80.0, 7.0, 0.05, 50.0, 1.003
# name -> (sampler, N, S_churn, guided, seed)
CHAINS = {"heun8": ("heun", 8, 0.0, False, 9201), "euler8": ("euler", 8, 0.0, False, 9202),
          "churn6": ("heun", 6, 1.8, False, 9203), "guided4": ("heun", 4, 0.0, True, 9204)}
GUIDED_CLASSES, GUIDED_SCALE = (0, 1, 2, 0), 3.0


class _TimePlusLabel(nn.Module):
    """in place of ``Unet.time_mlp``: the time embedding plus one row of the label embedding per sample"""

    def __init__(self, time_mlp, weight):
        super().__init__()
        self.time_mlp = time_mlp
        self.weight = nn.Parameter(weight.clone())
        self.classes = None

    def forward(self, t):
        return self.time_mlp(t) + self.weight[self.classes]


def coefficients(sigma):
    s2 = sigma ** 2 + SD ** 2
    return 1 / s2.sqrt(), sigma.log() / 4, SD ** 2 / s2, sigma * SD / s2.sqrt()


def denoise(net, x, sigma, clip=False):
    """(D, F, D before the clamp) at per-sample sigma [B], in the dtype of ``x``"""
    c_in, c_noise, c_skip, c_out = (c.view(-1, 1, 1, 1) for c in coefficients(sigma))
    F = net(c_in * x, c_noise.view(-1))
    D = c_skip * x + c_out * F
    return (D.clamp(-1.0, 1.0) if clip else D), F, D


def grid(N):
    a, b = SMAX ** (1 / RHO), SMIN ** (1 / RHO)
    g = [(a + i / (N - 1) * (b - a)) ** RHO for i in range(N)]
    g[0], g[-1] = SMAX, SMIN
    return g + [0.0]


def chain(fwd, dtype, kind, N, churn, init, noises):
    """Algorithm 2 in ``dtype`` -> (final image in the data range, steps with gamma > 0, steps in which the clamp acted)"""
    sig = grid(N)
    B = init.shape[0]
    full = lambda v: torch.full((B,), v, dtype=dtype)  # noqa: E731
    x = init.to(dtype) * torch.tensor(sig[0], dtype=dtype)
    churned = clamped = 0
    for i in range(N):
        gamma = min(churn / N, math.sqrt(2) - 1) if S_TMIN <= sig[i] <= S_TMAX else 0.0
        hat = sig[i] * (1 + gamma)
        if gamma > 0:
            churned += 1
            x = x + torch.tensor(math.sqrt(hat ** 2 - sig[i] ** 2) * S_NOISE, dtype=dtype) * noises[i].to(dtype)
        D, _, raw = fwd(x, full(hat))
        acted = bool((raw.abs() > 1).any())
        d = (x - D) / torch.tensor(hat, dtype=dtype)
        dt = torch.tensor(sig[i + 1] - hat, dtype=dtype)
        xp = x + dt * d
        if kind == "heun" and sig[i + 1] > 0:
            D2, _, raw2 = fwd(xp, full(sig[i + 1]))
            acted = acted or bool((raw2.abs() > 1).any())
            d2 = (xp - D2) / torch.tensor(sig[i + 1], dtype=dtype)
            xp = x + dt * ((d + d2) / 2)
        clamped += int(acted)
        x = xp
    return (x.clamp(-1.0, 1.0) + 1) * 0.5, churned, clamped


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B = 16, 16, 4
    g = torch.Generator().manual_seed(101)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)
    ge = torch.Generator().manual_seed(EXTRA_SEED)
    bound = 1.0 / math.sqrt(17)
    extra = {"time_mlp.0.weights": torch.randn(8, generator=ge),
             "time_mlp.1.weight": (torch.rand(64, 17, generator=ge) * 2 - 1) * bound,
             "time_mlp.1.bias": (torch.rand(64, generator=ge) * 2 - 1) * bound}
    label_emb = torch.randn(K + 1, 64, generator=ge)
    weights = dict(O.unet_init(dim=dim, channels=3, seed=SEED))
    weights.update(extra)
    fx = {"dim": dim, "S": S, "B": B, "data_seed": 101, "seed": SEED, "extra_seed": EXTRA_SEED, "K": K, "sigma": np.asarray(SIGMAS),
          "sigma_data": SD, "sigma_min": SMIN, "sigma_max": SMAX, "rho": RHO, "S_tmin": S_TMIN, "S_tmax": S_TMAX, "S_noise": S_NOISE,
          "grad_sample": SAMPLE, "label_emb.weight": label_emb.numpy(), "chains": np.asarray(sorted(CHAINS)),
          "guided_classes": np.asarray(GUIDED_CLASSES), "guided_scale": GUIDED_SCALE}
    for k, v in extra.items():
        fx[k] = v.numpy()

    def network(double=False, random=False, labels=False):
        net = R.Unet(dim=dim, channels=3, **(dict(random_fourier_features=True) if random else dict(learned_sinusoidal_cond=True)))
        net.load_state_dict(weights, strict=True)
        if labels:
            net.time_mlp = _TimePlusLabel(net.time_mlp, label_emb)
        return net.double() if double else net

    for tag, random in (("learned", False), ("random", True)):
        net = network(random=random)
        fx[f"{tag}:keys"] = np.asarray(list(net.state_dict().keys()))
        fx[f"{tag}:shapes"] = np.asarray([",".join(map(str, v.shape)) for v in net.state_dict().values()])
        fx[f"{tag}:param_order"] = np.asarray([n for n, _ in net.named_parameters()])
        fx[f"{tag}:requires_grad:time_mlp.0.weights"] = bool(net.time_mlp[0].weights.requires_grad)

    # the loss in its textbook form and every gradient, float32; the same in float64
    sigma = torch.tensor(SIGMAS)
    y = img * 2 - 1
    for tag, random in (("learned", False), ("random", True)):
        net = network(random=random)
        x = y + sigma.view(-1, 1, 1, 1) * noise
        D, F, _ = denoise(net, x, sigma)
        lam = (sigma ** 2 + SD ** 2) / (sigma * SD) ** 2
        loss = (lam * ((D - y) ** 2).reshape(B, -1).mean(1)).mean()
        loss.backward()
        fx[f"{tag}:F"], fx[f"{tag}:loss"] = F.detach().numpy(), loss.detach().numpy()
        for n, p in net.named_parameters():
            if p.grad is None:
                assert random and n == "time_mlp.0.weights", n
                continue
            flat = p.grad.reshape(-1)
            if flat.numel() <= WHOLE:
                fx[f"{tag}:grad:{n}"] = p.grad.numpy().copy()
            else:
                fx[f"{tag}:gradnorm:{n}"] = np.float64(flat.double().norm().item())
                fx[f"{tag}:gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[f"{tag}:gradnorm_all"] = np.float64(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters()
                                                                if p.grad is not None)).item())
        n64 = network(True, random)
        with torch.no_grad():
            x64 = y.double() + sigma.double().view(-1, 1, 1, 1) * noise.double()
            D64, F64, _ = denoise(n64, x64, sigma.double())
            loss64 = (lam.double() * ((D64 - y.double()) ** 2).reshape(B, -1).mean(1)).mean()
        fx[f"{tag}:F64"], fx[f"{tag}:loss64"] = F64.numpy(), loss64.numpy()
        print(f"{tag}: loss {float(loss.detach()):.6f} (float64 {float(loss64):.6f})")
    fx["x"] = (y + sigma.view(-1, 1, 1, 1) * noise).numpy()

    # chains
    for name, (kind, N, churn, guided, seed) in CHAINS.items():
        gc = torch.Generator().manual_seed(seed)
        init = torch.randn(B, 3, S, S, generator=gc)
        noises = [torch.randn(B, 3, S, S, generator=gc) for _ in range(N)]
        out = {}
        for dtype in (torch.float32, torch.float64):
            net = network(dtype == torch.float64, labels=guided)

            def fwd(x, s, net=net):
                if not guided:
                    return denoise(net, x, s, clip=True)
                net.time_mlp.classes = torch.tensor(GUIDED_CLASSES)
                c_in, c_noise, c_skip, c_out = (c.view(-1, 1, 1, 1) for c in coefficients(s))
                cond = net(c_in * x, c_noise.view(-1))
                net.time_mlp.classes = torch.full((B,), K)
                null = net(c_in * x, c_noise.view(-1))
                raw = c_skip * x + c_out * (null + GUIDED_SCALE * (cond - null))
                return raw.clamp(-1.0, 1.0), None, raw

            with torch.no_grad():
                out[dtype] = chain(fwd, dtype, kind, N, churn, init, noises)
        im32, churned, clamped = out[torch.float32]
        im64 = out[torch.float64][0]
        dist = float((im32.double() - im64).abs().max() / im64.abs().max())
        assert clamped >= 1, (name, "the clamp never acts")
        if churn > 0:
            assert 2 * churned >= N, (name, churned)
        fx[f"{name}:init"] = init.numpy()
        if churn > 0:                                        # (no other chain reads its noises)
            fx[f"{name}:noises"] = torch.stack(noises).numpy()
        fx[f"{name}:image"], fx[f"{name}:image64"] = im32.numpy(), im64.numpy()
        fx[f"{name}:dist"], fx[f"{name}:churned"], fx[f"{name}:clamped"] = np.float64(dist), churned, clamped
        fx[f"{name}:spec"] = np.asarray([kind, str(N), repr(churn), str(int(guided))])
        print(f"{name}: float32 vs float64 {dist:.3e}, gamma > 0 on {churned} of {N} steps, clamp acted in {clamped}")
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
