"""The MLP VAE restated in plain torch, in whatever dtype its operands have (float64 in the tests): forward, the L1 + KLD
loss and every gradient written out by hand (no autograd), plus the seeded weights the fixture tool and the tests share.
Weights are a state dict with the reference's keys (``encoder.layers.{0,2,4}``, ``encoder.mu``, ``encoder.log_var``,
``decoder.layers.{0,2,4,6}``)."""
import numpy as np
import torch

SLOPE = 0.2
HIDDEN = (512, 256, 128)
KEYS = [f"{m}.{p}" for m in ("encoder.layers.0", "encoder.layers.2", "encoder.layers.4", "encoder.mu", "encoder.log_var",
                             "decoder.layers.0", "decoder.layers.2", "decoder.layers.4", "decoder.layers.6")
        for p in ("weight", "bias")]

# (B, K, N) of the dense kernel tests (tests/test_hip_vae.py on the device, tests/test_vae_host.py their CPU scores)
DENSE_SHAPES = [(1, 64, 512), (3, 12, 8), (33, 784, 512), (32, 512, 784), (32, 4, 128), (130, 20, 128), (3, 25, 512),
                (3, 512, 25), (5, 128, 3), (512, 256, 512)]


def layer_sizes(img_channels: int, img_size: int, latent_dim: int):
    """{module name: (fan_in, fan_out)} in parameter order"""
    D = img_channels * img_size * img_size
    h0, h1, h2 = HIDDEN
    return {"encoder.layers.0": (D, h0), "encoder.layers.2": (h0, h1), "encoder.layers.4": (h1, h2),
            "encoder.mu": (h2, latent_dim), "encoder.log_var": (h2, latent_dim),
            "decoder.layers.0": (latent_dim, h2), "decoder.layers.2": (h2, h1), "decoder.layers.4": (h1, h0),
            "decoder.layers.6": (h0, D)}


def vae_init(img_channels: int, img_size: int, latent_dim: int, seed: int):
    """A float32 state dict in the reference's key order from ``np.random.RandomState(seed)``: weights and biases uniform in
    +-1 / sqrt(fan_in), the scale of torch's default ``nn.Linear`` initialisation"""
    rs = np.random.RandomState(seed)
    P = {}
    for name, (fin, fout) in layer_sizes(img_channels, img_size, latent_dim).items():
        b = 1.0 / np.sqrt(fin)
        P[f"{name}.weight"] = torch.from_numpy(rs.uniform(-b, b, size=(fout, fin)).astype(np.float32))
        P[f"{name}.bias"] = torch.from_numpy(rs.uniform(-b, b, size=(fout,)).astype(np.float32))
    return P


def lrelu(v):
    return torch.where(v > 0, v, v * SLOPE)


def encode(P, x):
    """x [B, C, S, S] -> (mu, log_var, [inputs of the three layers + h], [their pre-activations])"""
    a, acts, pres = x.reshape(x.shape[0], -1), [], []
    for i in (0, 2, 4):
        acts.append(a)
        pre = a @ P[f"encoder.layers.{i}.weight"].T + P[f"encoder.layers.{i}.bias"]
        pres.append(pre)
        a = lrelu(pre)
    acts.append(a)
    mu = a @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = a @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    return mu, lv, acts, pres


def decode(P, z):
    """z [B, L] -> (x_hat [B, D], [inputs of the four layers], [pre-activations of the four layers])"""
    a, acts, pres = z, [], []
    for i in (0, 2, 4, 6):
        acts.append(a)
        pre = a @ P[f"decoder.layers.{i}.weight"].T + P[f"decoder.layers.{i}.bias"]
        pres.append(pre)
        a = lrelu(pre) if i != 6 else torch.tanh(pre)
    return a, acts, pres


def forward(P, x, eps, kld_weight: float):
    """-> dict(mu, log_var, z, x_hat [B, D], recon, kld, loss) and the tape ``backward`` reads"""
    mu, lv, eacts, epres = encode(P, x)
    z = mu + eps * torch.exp(lv / 2)
    xh, dacts, dpres = decode(P, z)
    x2 = x.reshape(x.shape[0], -1)
    recon = (xh - x2).abs().mean()
    kld = -0.5 * (1 + lv - mu ** 2 - lv.exp()).mean()
    out = dict(mu=mu, log_var=lv, z=z, x_hat=xh, recon=recon, kld=kld, loss=recon + kld_weight * kld)
    return out, (x2, eps, eacts, epres, dacts, dpres, out)


def backward(P, tape, kld_weight: float, gloss: float = 1.0):
    """{parameter name: gradient of gloss * loss}, by the chain rule written out"""
    x2, eps, eacts, epres, dacts, dpres, o = tape
    mu, lv, xh = o["mu"], o["log_var"], o["x_hat"]
    G = {}
    g = gloss * torch.sign(xh - x2) / xh.numel() * (1 - xh ** 2)
    for n, i in ((3, 6), (2, 4), (1, 2), (0, 0)):
        if i != 6:
            g = g * torch.where(dpres[n] > 0, torch.ones_like(g), torch.full_like(g, SLOPE))
        G[f"decoder.layers.{i}.weight"] = g.T @ dacts[n]
        G[f"decoder.layers.{i}.bias"] = g.sum(0)
        g = g @ P[f"decoder.layers.{i}.weight"]
    gz = g
    c = kld_weight * gloss / mu.numel()
    gmu = gz + c * mu
    glv = gz * eps * 0.5 * torch.exp(lv / 2) + c * 0.5 * (lv.exp() - 1)
    h = eacts[3]
    G["encoder.mu.weight"], G["encoder.mu.bias"] = gmu.T @ h, gmu.sum(0)
    G["encoder.log_var.weight"], G["encoder.log_var.bias"] = glv.T @ h, glv.sum(0)
    g = gmu @ P["encoder.mu.weight"] + glv @ P["encoder.log_var.weight"]
    for n, i in ((2, 4), (1, 2), (0, 0)):
        g = g * torch.where(epres[n] > 0, torch.ones_like(g), torch.full_like(g, SLOPE))
        G[f"encoder.layers.{i}.weight"] = g.T @ eacts[n]
        G[f"encoder.layers.{i}.bias"] = g.sum(0)
        g = g @ P[f"encoder.layers.{i}.weight"]
    return G


def kink_margin(tape) -> float:
    """The smallest distance of a LeakyReLU input or an ``x_hat - x`` of this forward from zero"""
    x2, _, _, epres, _, dpres, o = tape
    vals = [p.abs().min() for p in epres] + [p.abs().min() for p in dpres[:3]] + [(o["x_hat"] - x2).abs().min()]
    return float(torch.stack(vals).min())


def fixture_grad_error(fx, case, name, got) -> float:
    """relative distance of a gradient (any float tensor of the parameter's shape) from the fixture's record of it"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    pre = f"{case}:"
    if f"{pre}grad:{name}" in fx:
        want = torch.from_numpy(fx[f"{pre}grad:{name}"]).double()
        return float((got - want).norm() / want.norm())
    n = int(fx["grad_sample"])
    want = torch.from_numpy(fx[f"{pre}gradsample:{name}"]).double()
    err_s = float((got[:: got.numel() // n][:n] - want).norm() / want.norm())
    norm = float(fx[f"{pre}gradnorm:{name}"])
    return max(err_s, abs(float(got.norm()) - norm) / norm)
