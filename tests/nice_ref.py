"""NICE restated in plain torch, in whatever dtype its operands have (float64 or float32 in the tests): the forward, the
inverse, the loss under both signs of the log-determinant, the exact log-density and every gradient written out by hand (no
autograd), and the seeded weights the fixture tool and the tests share.  Weights are a state dict with the reference's keys
(``layers.{i}.transformation.net.{0,2}``, ``scaling_layer.log_scale`` last)."""
import math

import numpy as np
import torch

SLOPE = 0.2
LOG_2PI = math.log(2.0 * math.pi)
LS = "scaling_layer.log_scale"


def net_name(i: int, j: int) -> str:
    return f"layers.{i}.transformation.net.{j}"


def keys(n_layers: int):
    """the reference's state_dict keys = its parameter order"""
    return [f"{net_name(i, j)}.{p}" for i in range(n_layers) for j in (0, 2) for p in ("weight", "bias")] + [LS]


def shapes(dim: int, n_layers: int, hidden: int):
    half = dim // 2
    out = {}
    for i in range(n_layers):
        out[f"{net_name(i, 0)}.weight"], out[f"{net_name(i, 0)}.bias"] = [hidden, half], [hidden]
        out[f"{net_name(i, 2)}.weight"], out[f"{net_name(i, 2)}.bias"] = [half, hidden], [half]
    out[LS] = [dim]
    return out


def nice_init(dim: int, n_layers: int, hidden: int, seed: int, log_scale_std: float = 0.3):
    """A float32 state dict in the reference's key order from ``np.random.RandomState(seed)``: weights and biases uniform in
    +-1 / sqrt(fan_in), the scale of torch's default ``nn.Linear`` initialisation; log_scale normal with the given deviation
    (the module's own zeros would leave the scaling layer out of every check)"""
    rs = np.random.RandomState(seed)
    half = dim // 2
    P = {}
    for i in range(n_layers):
        for j, (fin, fout) in ((0, (half, hidden)), (2, (hidden, half))):
            b = 1.0 / np.sqrt(fin)
            P[f"{net_name(i, j)}.weight"] = torch.from_numpy(rs.uniform(-b, b, size=(fout, fin)).astype(np.float32))
            P[f"{net_name(i, j)}.bias"] = torch.from_numpy(rs.uniform(-b, b, size=(fout,)).astype(np.float32))
    P[LS] = torch.from_numpy((log_scale_std * rs.standard_normal(dim)).astype(np.float32))
    return P


def n_layers_of(P) -> int:
    return (len(P) - 1) // 4


def lrelu(v):
    return torch.where(v > 0, v, SLOPE * v)


def halves(i: int, half: int, alternate: bool):
    """(conditioning lanes, shifted lanes) of layer i"""
    lo, hi = slice(0, half), slice(half, 2 * half)
    return (hi, lo) if alternate and i % 2 == 1 else (lo, hi)


def net(P, i, xc):
    """-> (t, the hidden pre-activation, the hidden activation)"""
    pre = xc @ P[f"{net_name(i, 0)}.weight"].T + P[f"{net_name(i, 0)}.bias"]
    a = lrelu(pre)
    return a @ P[f"{net_name(i, 2)}.weight"].T + P[f"{net_name(i, 2)}.bias"], pre, a


def forward(P, x, alternate: bool = False, exact: bool = False):
    """x [B, D] -> dict(h (the state before the scaling layer), z, mean_ll, sum_ls, loss, log_prob [B]) and the tape"""
    L, half = n_layers_of(P), x.shape[1] // 2
    states, pres, acts = [x], [], []
    for i in range(L):
        c, s = halves(i, half, alternate)
        t, pre, a = net(P, i, states[-1][:, c])
        nxt = states[-1].clone()
        nxt[:, s] = states[-1][:, s] + t
        states.append(nxt)
        pres.append(pre)
        acts.append(a)
    ls = P[LS]
    z = states[-1] * torch.exp(ls)
    D = x.shape[1]
    ll = -0.5 * (z ** 2).sum(1) - 0.5 * D * LOG_2PI
    mean_ll, sum_ls = ll.mean(), ls.sum()
    loss = -(mean_ll + sum_ls) if exact else -(mean_ll - sum_ls)
    out = dict(h=states[-1], z=z, mean_ll=mean_ll, sum_ls=sum_ls, loss=loss, log_prob=ll + sum_ls)
    return out, (states, pres, acts, z, alternate, exact)


def inverse(P, z, alternate: bool = False):
    L, half = n_layers_of(P), z.shape[1] // 2
    x = z * torch.exp(-P[LS])
    for i in range(L - 1, -1, -1):
        c, s = halves(i, half, alternate)
        t, _, _ = net(P, i, x[:, c])
        nxt = x.clone()
        nxt[:, s] = x[:, s] - t
        x = nxt
    return x


def backward(P, tape, gloss: float = 1.0):
    """{parameter name: gradient of gloss * loss}, by the chain rule written out"""
    states, pres, acts, z, alternate, exact = tape
    B, D = z.shape
    half = D // 2
    ls = P[LS]
    G = {}
    gz = (gloss / B) * z                                    # d(-mean_ll) / dz
    G[LS] = (gz * z).sum(0) + (-gloss if exact else gloss)  # z = h e^s: dz / ds = z
    g = gz * torch.exp(ls)
    for i in range(n_layers_of(P) - 1, -1, -1):
        c, s = halves(i, half, alternate)
        gt = g[:, s]
        G[f"{net_name(i, 2)}.weight"] = gt.T @ acts[i]
        G[f"{net_name(i, 2)}.bias"] = gt.sum(0)
        ga = (gt @ P[f"{net_name(i, 2)}.weight"]) * torch.where(pres[i] > 0, torch.ones_like(pres[i]),
                                                                 torch.full_like(pres[i], SLOPE))
        G[f"{net_name(i, 0)}.weight"] = ga.T @ states[i][:, c]
        G[f"{net_name(i, 0)}.bias"] = ga.sum(0)
        g = g.clone()
        g[:, c] = g[:, c] + ga @ P[f"{net_name(i, 0)}.weight"]
    return G


def kink_values(tape):
    """every LeakyReLU input of a forward, flattened"""
    return torch.cat([p.reshape(-1) for p in tape[1]])


def kink_margin(tape) -> float:
    """The smallest distance of a LeakyReLU input of this forward from zero"""
    return float(kink_values(tape).abs().min())


def max_state(tape) -> float:
    """the largest absolute value of any state of a forward (z included)"""
    return max(float(s.abs().max()) for s in list(tape[0]) + [tape[3]])


def fixture_grad_error(fx, case, name, got) -> float:
    """relative distance of a gradient (any float tensor of the parameter's shape) from the fixture's record of it"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    want = torch.from_numpy(fx[f"{case}:grad:{name}"]).double().reshape(-1)
    return float((got - want).norm() / want.norm())
