"""The denoising autoencoder restated in plain torch, in whatever dtype its operands have (float64 or float32 in the tests):
the corruption from given draws, the forward, the MSE loss and every gradient written out by hand (no autograd), the numpy
restatement of the Philox mask of csrc/dae.hip, and the seeded weights the fixture tool and the tests share.  Weights are a
state dict with the reference's keys (``encoder.model.{0,2}``, ``decoder.model.{0,2}``)."""
import numpy as np
import torch

import dropout_ref as DR

HIDDEN, CODE = 256, 128
LAYERS = ("encoder.model.0", "encoder.model.2", "decoder.model.0", "decoder.model.2")
KEYS = [f"{m}.{p}" for m in LAYERS for p in ("weight", "bias")]
MODES = {"salt_and_pepper": 0, "masking": 1}


def layer_sizes(img_channels: int, img_size: int):
    """{module name: (fan_in, fan_out)} in parameter order"""
    D = img_channels * img_size * img_size
    return {LAYERS[0]: (D, HIDDEN), LAYERS[1]: (HIDDEN, CODE), LAYERS[2]: (CODE, HIDDEN), LAYERS[3]: (HIDDEN, D)}


def dae_init(img_channels: int, img_size: int, seed: int):
    """A float32 state dict in the reference's key order from ``np.random.RandomState(seed)``: weights and biases uniform in
    +-1 / sqrt(fan_in), the scale of torch's default ``nn.Linear`` initialisation"""
    rs = np.random.RandomState(seed)
    P = {}
    for name, (fin, fout) in layer_sizes(img_channels, img_size).items():
        b = 1.0 / np.sqrt(fin)
        P[f"{name}.weight"] = torch.from_numpy(rs.uniform(-b, b, size=(fout, fin)).astype(np.float32))
        P[f"{name}.bias"] = torch.from_numpy(rs.uniform(-b, b, size=(fout,)).astype(np.float32))
    return P


# ---- corruption ------------------------------------------------------------------------------------------------------------
def corrupt(x, noise_type: str, level: float, draws):
    """The reference's formulas from given draws: the normal draw (gaussian), (salt, pepper) uniform draws
    (salt_and_pepper), the uniform draw (masking)"""
    if noise_type == "gaussian":
        return x + draws * level
    if noise_type == "salt_and_pepper":
        salt, pepper = draws
        x = torch.where(salt < level / 2, torch.ones_like(x), x)
        return torch.where(pepper < level / 2, torch.zeros_like(x), x)
    if noise_type == "masking":
        return torch.where(draws < level, torch.zeros_like(x), x)
    raise ValueError(noise_type)


def mask_threshold(mode: str, level: float) -> int:
    p = float(level) / 2.0 if mode == "salt_and_pepper" else float(level)
    return min(2 ** 32 - 1, int(np.floor(p * 2.0 ** 32)))


def mask_words(n: int, key: int):
    """(w_s, w_p): uint64 [n] holding the 32-bit Philox words of logical elements 0 .. n - 1 under the 64-bit ``key``:
    element i takes word i & 3 of the call with counter (q lo, q hi, pass, 0), q = i >> 2; pass 0 salt, pass 1 pepper"""
    key = int(key) & (2 ** 64 - 1)
    k = (key & DR.MASK32, key >> 32)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    lo, hi = q & np.uint64(DR.MASK32), q >> np.uint64(32)
    return tuple(np.stack(DR.philox4x32_10((lo, hi, p, 0), k), axis=1).reshape(-1)[:n] for p in (0, 1))


def corrupt_mask(x, key: int, mode: str, level: float):
    """numpy float32 [B, D] -> what lgm_dae_corrupt_mask writes (the live lanes)"""
    x = np.asarray(x, dtype=np.float32)
    ws, wp = (w.reshape(x.shape) for w in mask_words(x.size, key))
    thr = np.uint64(mask_threshold(mode, level))
    if mode == "masking":
        return np.where(ws < thr, np.float32(0), x).astype(np.float32)
    return np.where(wp < thr, np.float32(0), np.where(ws < thr, np.float32(1), x)).astype(np.float32)


# ---- the network -----------------------------------------------------------------------------------------------------------
def relu(v):
    return torch.where(v > 0, v, torch.zeros_like(v))


def encode(P, xc):
    """xc [B, ...] -> (code [B, 128], [inputs of the two layers], [their pre-activations])"""
    a, acts, pres = xc.reshape(xc.shape[0], -1), [], []
    for n in LAYERS[:2]:
        acts.append(a)
        pres.append(a @ P[f"{n}.weight"].T + P[f"{n}.bias"])
        a = relu(pres[-1])
    return a, acts, pres


def decode(P, h):
    """h [B, 128] -> (x_hat [B, D], [inputs of the two layers], [their pre-activations])"""
    acts, pres = [h], [h @ P[f"{LAYERS[2]}.weight"].T + P[f"{LAYERS[2]}.bias"]]
    acts.append(relu(pres[0]))
    pres.append(acts[1] @ P[f"{LAYERS[3]}.weight"].T + P[f"{LAYERS[3]}.bias"])
    return torch.tanh(pres[1]), acts, pres


def forward(P, x, xc):
    """x the clean batch, xc its corrupted copy -> dict(code, x_hat [B, D], loss) and the tape ``backward`` reads"""
    h, eacts, epres = encode(P, xc)
    xh, dacts, dpres = decode(P, h)
    x2 = x.reshape(x.shape[0], -1)
    out = dict(code=h, x_hat=xh, loss=((x2 - xh) ** 2).mean())
    return out, (x2, eacts + dacts, epres + dpres, out)


def backward(P, tape, gloss: float = 1.0):
    """{parameter name: gradient of gloss * loss}, by the chain rule written out"""
    x2, acts, pres, o = tape
    xh = o["x_hat"]
    g = (2.0 * gloss / xh.numel()) * (xh - x2) * (1 - xh ** 2)
    G = {}
    for i in (3, 2, 1, 0):
        if i != 3:
            g = g * torch.where(pres[i] > 0, torch.ones_like(g), torch.zeros_like(g))
        G[f"{LAYERS[i]}.weight"] = g.T @ acts[i]
        G[f"{LAYERS[i]}.bias"] = g.sum(0)
        g = g @ P[f"{LAYERS[i]}.weight"]
    return G


def kink_values(tape):
    """every ReLU input of a forward, flattened"""
    return torch.cat([p.reshape(-1) for p in tape[2][:3]])


def kink_margin(tape) -> float:
    """The smallest distance of a ReLU input of this forward from zero"""
    return float(kink_values(tape).abs().min())


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
