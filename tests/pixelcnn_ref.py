"""The gated PixelCNN restated in plain torch, in whatever dtype its operands have (float64 in the tests): the masks, the
network, the cross-entropy, the inverse-CDF draw and the chain of ``sample``.  Weights are a state dict with the reference's
keys (``input_conv.weight``, ``gated_blocks.<i>.conv.weight``, ``output_conv.weight``, ... ); masks are applied here, so
a dead tap's value never matters."""
import torch
import torch.nn.functional as F


def live_taps(k: int, mask_type: str) -> int:
    return (k // 2) * k + k // 2 + (1 if mask_type == "B" else 0)


def mask(k: int, mask_type: str, dtype=torch.float64) -> torch.Tensor:
    """[k, k]: 1 on the taps whose row-major index is below ``live_taps``"""
    return (torch.arange(k * k) < live_taps(k, mask_type)).to(dtype).view(k, k)


def init(cin: int, hid: int, K: int, layers: int, seed: int):
    """A float32 state dict in the reference's key order (masks included, dead taps zero), drawn from ``seed``: normal weights
    scaled so that the gates' pre-activations and the logits are of order one"""
    g = torch.Generator().manual_seed(seed)
    P = {}

    def conv(name, cout, cin_, k, mask_type, gain):
        live = live_taps(k, mask_type) if mask_type else k * k
        w = torch.randn(cout, cin_, k, k, generator=g) * (gain / (live * cin_) ** 0.5)
        P[f"{name}.weight"] = w * mask(k, mask_type, torch.float32) if mask_type else w
        P[f"{name}.bias"] = torch.randn(cout, generator=g) * 0.1
        if mask_type:
            P[f"{name}.mask"] = mask(k, mask_type, torch.float32).expand(cout, cin_, k, k).clone()

    conv("input_conv", hid, cin, 7, "A", 1.5)
    for i in range(layers):
        conv(f"gated_blocks.{i}.conv", 2 * hid, hid, 7, "B", 1.5)
    conv("output_conv", K, hid, 1, None, 2.0)
    return P


def masked_conv(x, w, b, mask_type: str):
    k = w.shape[-1]
    return F.conv2d(x, w * mask(k, mask_type, w.dtype), b, padding=k // 2)


def gate(x, pre):
    a, b = torch.chunk(pre, 2, dim=1)
    return x + torch.tanh(a) * torch.sigmoid(b)


def num_layers(P) -> int:
    return 1 + max(int(k.split(".")[1]) for k in P if k.startswith("gated_blocks."))


def forward(P, x):
    """x [B, C, H, W] -> logits [B, K, H, W]"""
    h = masked_conv(x, P["input_conv.weight"], P["input_conv.bias"], "A")
    for i in range(num_layers(P)):
        h = gate(h, masked_conv(h, P[f"gated_blocks.{i}.conv.weight"], P[f"gated_blocks.{i}.conv.bias"], "B"))
    return F.conv2d(h, P["output_conv.weight"], P["output_conv.bias"])


def loss(P, x, target):
    return F.cross_entropy(forward(P, x), target)


def draw(logits, u, temperature: float = 1.0):
    """logits [B, K], u [B] -> the first class whose cumulative probability exceeds u, clamped to the last class with p > 0"""
    p = torch.softmax(logits / temperature, dim=-1)
    cdf = torch.cumsum(p, dim=-1)
    over = cdf > u.to(cdf.dtype).unsqueeze(-1)
    K = logits.shape[-1]
    first = torch.where(over.any(-1), over.to(torch.int64).argmax(-1), torch.full_like(over[:, 0], K, dtype=torch.int64))
    last_pos = (K - 1) - (p > 0).flip(-1).to(torch.int64).argmax(-1)
    return torch.minimum(first, last_pos)


def chain(P, codebook, uniforms, h: int, w: int, temperature: float = 1.0):
    """uniforms [h * w, B]; codebook [K, C] or None (the index as a float in every channel) -> (codes [B, h, w], the logits
    [h * w, B, K] each position was drawn from).  A whole forward per position: the definition, not the fast way."""
    B = uniforms.shape[1]
    C = P["input_conv.weight"].shape[1]
    dtype = P["input_conv.weight"].dtype
    x = torch.zeros(B, C, h, w, dtype=dtype)
    codes = torch.zeros(B, h, w, dtype=torch.int64)
    seen = []
    for p in range(h * w):
        i, j = divmod(p, w)
        lg = forward(P, x)[:, :, i, j]
        idx = draw(lg, uniforms[p], temperature)
        codes[:, i, j] = idx
        x[:, :, i, j] = codebook[idx].to(dtype) if codebook is not None else idx.to(dtype).unsqueeze(-1).expand(B, C)
        seen.append(lg)
    return codes, torch.stack(seen)


# ---- the three GEMMs of one masked layer, per element (oracle.bounds' operands with the mask applied) ------------------------
# (B, h, w, C, N, k, type)
CONV_SHAPES = [(1, 4, 4, 4, 8, 7, "A"), (3, 4, 4, 20, 40, 7, "B"), (2, 8, 8, 64, 128, 7, "B"), (3, 3, 10, 8, 16, 7, "A"),
               (2, 5, 6, 12, 24, 3, "B"), (2, 8, 8, 128, 256, 7, "B"), (1, 1, 1, 4, 8, 7, "B"),
               (36, 8, 8, 8, 16, 3, "B")]      # the last: 2304 positions, where the weight gradient splits into two runs


class ConvProblem:
    """float32 operands of one masked layer (``oracle.bounds.make_inputs``, the weight masked) and, per kernel, the float64
    result ``ref`` and the absolute-value result ``S``: xy = conv + bias; yx = conv^T + res; wgrad at beta = 1 (gw0 + masked
    gradient: a dead tap keeps gw0) and at beta = 0 (a dead tap is an exact zero), each followed by the bias gradient."""

    def __init__(self, shape):
        from oracle import bounds
        B, H, W, C, N, k, mt = shape
        self.shape, self.geom = shape, (B, H, W, C, N, k, 1, k // 2)
        self.L = live_taps(k, mt)
        self.t = bounds.make_inputs(self.geom)
        self.m = mask(k, mt, torch.float32)
        self.t["w"] = self.t["w"] * self.m
        self.n = {"xy": self.L * C, "yx": self.L * N, "wgrad1": B * H * W, "wgrad0": B * H * W}
        d = {k_: v.double() for k_, v in self.t.items()}
        a = {k_: v.abs() for k_, v in d.items()}
        self.ref = {kind: self.eval(kind, d) for kind in self.n}
        self.S = {kind: self.eval(kind, a) for kind in self.n}

    def eval(self, kind, t):
        from oracle import bounds
        if kind == "xy":
            return bounds.conv_xy(self.geom, t["x"], t["w"], t["b"])
        if kind == "yx":
            return bounds.conv_yx(self.geom, t["gy"], t["w"], None, t["res_x"])
        gw, gb = bounds.conv_wgrad(self.geom, t["gy"], t["x"])
        gw = gw * self.m.to(gw.dtype)
        if kind == "wgrad1":
            gw, gb = gw + t["gw0"], gb + t["gb0"]
        return torch.cat([gw.reshape(-1), gb.reshape(-1)])

    def score(self, kind, got):
        from oracle import bounds
        return bounds.forward_error_units(got, self.ref[kind], self.S[kind])
