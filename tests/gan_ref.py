"""The MLP GAN restated in plain torch, in whatever dtype its operands have (float64 in the tests): the seeded weights the
fixture tool and the tests share, the generator (Linear -> train-mode BatchNorm1d with its running-statistics update ->
LeakyReLU three times, Linear -> Tanh), the discriminator, the three losses of reference models/generative/gan/gan.py:258-308
and every gradient written out by hand (no autograd).  Weights are one state dict with the module's keys (``G.model.{0..9}``,
``D.model.{0,2,4}``)."""
import numpy as np
import torch

SLOPE = 0.2
EPS = 1e-5
MOMENTUM = 0.1
G_HIDDEN = (256, 512, 1024)
D_HIDDEN = (512, 256)
LOSS_TYPES = ("non-saturating", "min-max")

_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
G_KEYS = ([f"model.0.{p}" for p in ("weight", "bias")] + [f"model.1.{p}" for p in _BN]
          + [f"model.3.{p}" for p in ("weight", "bias")] + [f"model.4.{p}" for p in _BN]
          + [f"model.6.{p}" for p in ("weight", "bias")] + [f"model.7.{p}" for p in _BN]
          + [f"model.9.{p}" for p in ("weight", "bias")])
D_KEYS = [f"model.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
KEYS = [f"G.{k}" for k in G_KEYS] + [f"D.{k}" for k in D_KEYS]
G_PARAMS = [k for k in G_KEYS if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]

# (B, F) of the BatchNorm1d kernel tests and B of the loss-head tests (tests/test_hip_gan_mlp.py)
BN_SHAPES = [(B, F) for B in (2, 3, 16, 17, 33, 130) for F in (4, 6, 16, 36, 260)]
BCE_SIZES = (1, 5, 64, 130)


def g_sizes(img_channels, img_size, latent_dim):
    D = img_channels * img_size * img_size
    return [(0, latent_dim, G_HIDDEN[0]), (3, G_HIDDEN[0], G_HIDDEN[1]), (6, G_HIDDEN[1], G_HIDDEN[2]), (9, G_HIDDEN[2], D)]


def d_sizes(img_channels, img_size):
    D = img_channels * img_size * img_size
    return [(0, D, D_HIDDEN[0]), (2, D_HIDDEN[0], D_HIDDEN[1]), (4, D_HIDDEN[1], 1)]


def gan_init(img_channels: int, img_size: int, latent_dim: int, seed: int):
    """A float32 state dict in the module's key order from ``np.random.RandomState(seed)``: Linear weights and biases uniform
    in +-1 / sqrt(fan_in) (the scale of torch's default), BatchNorm weights in (0.5, 1.5), biases and running means in
    (-0.5, 0.5), running variances in (0.5, 1.5) - away from the identity, so that every one of them is tested"""
    rs = np.random.RandomState(seed)
    P = {}

    def f32(a):
        return torch.from_numpy(np.asarray(a).astype(np.float32))
    for i, fin, fout in g_sizes(img_channels, img_size, latent_dim):
        b = 1.0 / np.sqrt(fin)
        P[f"G.model.{i}.weight"] = f32(rs.uniform(-b, b, size=(fout, fin)))
        P[f"G.model.{i}.bias"] = f32(rs.uniform(-b, b, size=(fout,)))
        if i != 9:
            P[f"G.model.{i + 1}.weight"] = f32(rs.uniform(0.5, 1.5, size=(fout,)))
            P[f"G.model.{i + 1}.bias"] = f32(rs.uniform(-0.5, 0.5, size=(fout,)))
            P[f"G.model.{i + 1}.running_mean"] = f32(rs.uniform(-0.5, 0.5, size=(fout,)))
            P[f"G.model.{i + 1}.running_var"] = f32(rs.uniform(0.5, 1.5, size=(fout,)))
            P[f"G.model.{i + 1}.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    for i, fin, fout in d_sizes(img_channels, img_size):
        b = 1.0 / np.sqrt(fin)
        P[f"D.model.{i}.weight"] = f32(rs.uniform(-b, b, size=(fout, fin)))
        P[f"D.model.{i}.bias"] = f32(rs.uniform(-b, b, size=(fout,)))
    assert list(P) == KEYS
    return P


def to64(P):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}


def lrelu(v):
    return torch.where(v > 0, v, v * SLOPE)


def dlrelu(pre):
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))


# ---- BatchNorm1d --------------------------------------------------------------------------------------------------------
def bn_train(a, gamma, beta, eps=EPS):
    """-> (n = gamma xhat + beta, xhat, mean, biased var, rstd)"""
    mean = a.mean(0)
    var = ((a - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (a - mean) * rstd
    return gamma * xhat + beta, xhat, mean, var, rstd


def bn_running(rm, rv, mean, var, B, momentum=MOMENTUM):
    """torch's update: the running variance takes the unbiased batch variance"""
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * B / (B - 1)


def bn_eval(a, gamma, beta, rm, rv, eps=EPS):
    return gamma * ((a - rm) / torch.sqrt(rv + eps)) + beta


def bn_backward(g, xhat, gamma, rstd):
    """g: gradient at n -> (ga, ggamma, gbeta)"""
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    B = g.shape[0]
    return gamma * rstd * (g - s1 / B - xhat * s2 / B), s2, s1


# ---- the networks ---------------------------------------------------------------------------------------------------------
def g_forward(P, z, training: bool = True):
    """z [B, L] -> (x_hat [B, D], tape, {running statistic key: its value after this forward})"""
    h, tape, run = z, [], {}
    for i in (0, 3, 6):
        a = h @ P[f"G.model.{i}.weight"].T + P[f"G.model.{i}.bias"]
        bn = f"G.model.{i + 1}"
        if training:
            n, xhat, mean, var, rstd = bn_train(a, P[f"{bn}.weight"], P[f"{bn}.bias"])
            rm, rv = bn_running(P[f"{bn}.running_mean"], P[f"{bn}.running_var"], mean, var, z.shape[0])
            run[f"{bn}.running_mean"], run[f"{bn}.running_var"] = rm, rv
        else:
            n, xhat, rstd = bn_eval(a, P[f"{bn}.weight"], P[f"{bn}.bias"], P[f"{bn}.running_mean"], P[f"{bn}.running_var"]), None, None
        tape.append((h, xhat, rstd, n))
        h = lrelu(n)
    pre = h @ P["G.model.9.weight"].T + P["G.model.9.bias"]
    xh = torch.tanh(pre)
    tape.append((h, None, None, xh))
    return xh, tape, run


def g_backward(P, tape, gxh):
    """gxh [B, D]: gradient at x_hat -> {G parameter key (without the G. prefix): gradient}"""
    G = {}
    h, _, _, xh = tape[3]
    g = gxh * (1 - xh ** 2)
    G["model.9.weight"], G["model.9.bias"] = g.T @ h, g.sum(0)
    g = g @ P["G.model.9.weight"]
    for k, i in ((2, 6), (1, 3), (0, 0)):
        h_in, xhat, rstd, n = tape[k]
        ga, gg, gb = bn_backward(g * dlrelu(n), xhat, P[f"G.model.{i + 1}.weight"], rstd)
        G[f"model.{i + 1}.weight"], G[f"model.{i + 1}.bias"] = gg, gb
        G[f"model.{i}.weight"], G[f"model.{i}.bias"] = ga.T @ h_in, ga.sum(0)
        g = ga @ P[f"G.model.{i}.weight"]
    return G


def d_forward(P, x2):
    """x2 [B, D] -> (logits [B], tape)"""
    p1 = x2 @ P["D.model.0.weight"].T + P["D.model.0.bias"]
    a1 = lrelu(p1)
    p2 = a1 @ P["D.model.2.weight"].T + P["D.model.2.bias"]
    a2 = lrelu(p2)
    s = (a2 @ P["D.model.4.weight"].T + P["D.model.4.bias"])[:, 0]
    return s, (x2, p1, a1, p2, a2)


def d_backward(P, tape, gs):
    """gs [B]: gradient at the logits -> ({D parameter key: gradient}, gradient at x2)"""
    x2, p1, a1, p2, a2 = tape
    G = {}
    g = gs[:, None]
    G["model.4.weight"], G["model.4.bias"] = g.T @ a2, g.sum(0)
    g = (g @ P["D.model.4.weight"]) * dlrelu(p2)
    G["model.2.weight"], G["model.2.bias"] = g.T @ a1, g.sum(0)
    g = (g @ P["D.model.2.weight"]) * dlrelu(p1)
    G["model.0.weight"], G["model.0.bias"] = g.T @ x2, g.sum(0)
    return G, g @ P["D.model.0.weight"]


# ---- the losses -----------------------------------------------------------------------------------------------------------
def bce(s, t: float):
    """binary cross entropy with logits, per sample, in the stable form"""
    return s.clamp_min(0) - s * t + torch.log1p(torch.exp(-s.abs()))


def d_loss(P, x, x_hat, gloss: float = 1.0):
    """reference :258-283 -> (the five logged values, {D parameter key: gradient of gloss * d_loss})"""
    B = x.shape[0]
    s_r, t_r = d_forward(P, x.reshape(B, -1))
    s_f, t_f = d_forward(P, x_hat.reshape(B, -1))
    real, fake = bce(s_r, 1.0).mean(), bce(s_f, 0.0).mean()
    out = dict(d_loss=(real + fake) / 2, d_loss_real=real, d_loss_fake=fake, logits_real=s_r.mean(), logits_fake=s_f.mean(),
               s_real=s_r, s_fake=s_f)
    G_r, _ = d_backward(P, t_r, gloss * 0.5 * (torch.sigmoid(s_r) - 1) / B)
    G_f, _ = d_backward(P, t_f, gloss * 0.5 * torch.sigmoid(s_f) / B)
    return out, {k: G_r[k] + G_f[k] for k in G_r}


def g_loss(P, x_hat, loss_type: str, gloss: float = 1.0):
    """reference :285-308 -> (g_loss, mean logit, logits, gradient of gloss * g_loss at x_hat [B, D])"""
    B = x_hat.shape[0]
    s, tape = d_forward(P, x_hat.reshape(B, -1))
    if loss_type == "min-max":
        loss, gs = -bce(s, 0.0).mean(), -gloss * torch.sigmoid(s) / B
    else:
        loss, gs = bce(s, 1.0).mean(), gloss * (torch.sigmoid(s) - 1) / B
    return loss, s.mean(), s, d_backward(P, tape, gs)[1]


def kink_values(P, z, x):
    """every LeakyReLU input of one training step's forwards (G on z; D on x and on G(z)), flattened"""
    xh, tape, _ = g_forward(P, z, True)
    vals = [t[3].reshape(-1) for t in tape[:3]]
    for inp in (x.reshape(x.shape[0], -1), xh):
        _, (_, p1, _, p2, _) = d_forward(P, inp)
        vals += [p1.reshape(-1), p2.reshape(-1)]
    return torch.cat(vals)


def fixture_grad_error(fx, case, name, got) -> float:
    """relative distance of a gradient (any float tensor of the parameter's shape) from the fixture's record ``name`` of it"""
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
