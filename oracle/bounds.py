"""Elementwise forward-error check of the convolution family against float64 (CPU code, no GPU).

A float32 sum of products  y = sum_k a_k w_k (+ bias + residual)  computed in ANY order has the forward error
|y - y_exact| <= gamma * S with S = sum_k |a_k||w_k| (+ |bias| + |residual|): the error is measured in units of
2^-24 * S PER ELEMENT.  A ratio of Frobenius norms averages a local error (one dropped tap at one border pixel, one wrong
row of a ragged tile) over the whole tensor; this check does not.

The tolerance ``C`` is measured against the REFERENCE, never against the HIP kernels: tests/test_cpu_bounds.py evaluates every
shape of the kernel ledger (tests/test_hip_kernel_ledger.py) in float32 on the CPU, in torch's own order and with a strictly
sequential sum, and asserts that the worst score stays below ``C_REF_WORST``.  ``C`` is 4 times that: a kernel's summation
order (MFMA K-blocks, split-K planes, slabs) and operation count differ from the CPU's.  Per case the tolerance is capped
by the worst-case theorem 2 * (n + splits + 2) for a reduction of n terms (up to one ulp per operation, in case an
accumulator truncates)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

UNIT = 2.0 ** -24

# worst forward_error_units of a float32 CPU evaluation over every ledger shape, measured by tests/test_cpu_bounds.py:
# 8.56 in torch's own order (the 1x1 layer 192 -> 512 over 6208 pixels), 1.37 with the strictly sequential sum
# on a slice; rounded up.  The weakest mutation of any ledger shape scores 89.6.
C_REF_WORST = 9.0
C = 4.0 * C_REF_WORST


def tolerance(n: int) -> float:
    """The bound of one case in units of 2^-24 * S: the measured ``C``, capped by the theorem 2 * (n + splits + 2) for short
    reductions.  The cap is taken at splits = 1: more planes only widen it, and the unsplit form is the stricter one."""
    return min(C, 2.0 * (n + 1 + 2))


def forward_error_units(got, ref64, S64) -> float:
    """max_i |got_i - ref_i| / (2^-24 * S_i); where S_i == 0 (pad lanes, weight rows of pad channels) got_i must be
    exactly 0.  inf when that fails or when ``got`` holds a non-finite value."""
    got = got.detach().double().cpu()
    ref64, S64 = ref64.double(), S64.double()
    assert got.shape == ref64.shape == S64.shape, (got.shape, ref64.shape, S64.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    zero = S64 == 0
    if bool((got[zero] != 0).any()):
        return math.inf
    live = ~zero
    if not bool(live.any()):
        return 0.0
    return float(((got[live] - ref64[live]).abs() / (UNIT * S64[live])).max())


def rel(a, b) -> float:
    """The ratio of Frobenius norms the per-op tests use (informative here)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- the three GEMMs of a convolution layer as plain torch, in any dtype ------------------------------------------------
# geometry = (B, H, W, Cin, Cout, k, stride, pad); tensors are NCHW / OIHW with the TRUE channel counts

def out_hw(geom):
    B, H, W, Cin, Cout, k, s, p = geom
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def make_inputs(geom, seed=None):
    """Seeded float32 operands of one layer: x, w, b (over Cout), gy, bx (a bias over Cin for the input gradient), the
    residuals of both directions and a previous weight / bias gradient for the beta = 1 accumulate."""
    B, H, W, Cin, Cout, k, s, p = geom
    Ho, Wo = out_hw(geom)
    g = torch.Generator().manual_seed(sum(geom) if seed is None else seed)
    return {
        "x": torch.randn(B, Cin, H, W, generator=g),
        "w": torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k),
        "b": torch.randn(Cout, generator=g),
        "gy": torch.randn(B, Cout, Ho, Wo, generator=g),
        "bx": torch.randn(Cin, generator=g),
        "res_y": torch.randn(B, Cout, Ho, Wo, generator=g),
        "res_x": torch.randn(B, Cin, H, W, generator=g),
        "gw0": torch.randn(Cout, Cin, k, k, generator=g),
        "gb0": torch.randn(Cout, generator=g),
    }


def conv_xy(geom, x, w, b=None, res=None):
    y = F.conv2d(x, w, b, stride=geom[6], padding=geom[7])
    return y if res is None else y + res


def conv_yx(geom, gy, w, bx=None, res=None):
    B, H, W, Cin, Cout, k, s, p = geom
    Ho, Wo = out_hw(geom)
    op = (H - ((Ho - 1) * s - 2 * p + k), W - ((Wo - 1) * s - 2 * p + k))
    gx = F.conv_transpose2d(gy, w, bx, stride=s, padding=p, output_padding=op)
    return gx if res is None else gx + res


def conv_wgrad(geom, gy, x, gw0=None, gb0=None):
    """(gw, gb) = (beta * gw0 + sum_pixels gy x, beta * gb0 + sum_pixels gy) with beta = 1 where gw0 / gb0 are given."""
    B, H, W, Cin, Cout, k, s, p = geom
    gw = torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), gy, stride=s, padding=p)
    gb = gy.sum((0, 2, 3))
    return (gw if gw0 is None else gw + gw0), (gb if gb0 is None else gb + gb0)


def reduction_length(kind, geom) -> int:
    B, H, W, Cin, Cout, k, s, p = geom
    Ho, Wo = out_hw(geom)
    return {"xy": k * k * Cin, "yx": k * k * Cout, "wgrad": B * Ho * Wo}[kind]


class Problem:
    """One GEMM of one layer (kind = "xy" | "yx" | "wgrad") with every operand option switched on (bias, residual /
    previous gradient): float32 operands, the float64 result ``ref`` and the absolute-value result ``S``.  The weight
    gradient's result is the pair (gw, gb) flattened into one vector."""

    def __init__(self, kind, geom, seed=None):
        self.kind, self.geom = kind, tuple(geom)
        self.t = make_inputs(geom, seed)
        self.n = reduction_length(kind, geom)
        d = {k: v.double() for k, v in self.t.items()}
        a = {k: v.abs() for k, v in d.items()}
        self.ref, self.S = self._eval(d), self._eval(a)

    def _eval(self, t):
        if self.kind == "xy":
            return conv_xy(self.geom, t["x"], t["w"], t["b"], t["res_y"])
        if self.kind == "yx":
            return conv_yx(self.geom, t["gy"], t["w"], t["bx"], t["res_x"])
        gw, gb = conv_wgrad(self.geom, t["gy"], t["x"], t["gw0"], t["gb0"])
        return torch.cat([gw.reshape(-1), gb.reshape(-1)])

    def eval32(self):
        """float32 in torch's own order"""
        return self._eval(self.t)

    def score(self, got):
        return forward_error_units(got, self.ref, self.S)

    # -- one element as an explicit list of products -------------------------------------------------------------------
    def terms(self, idx):
        """(a, w, extra): float32 vectors with element ``idx`` = sum a * w + sum extra, in the natural order of the
        reduction (tap-major / channel-minor for the convolutions, pixel order for the weight gradient), plus per term
        the tap it belongs to (convolutions) or the pixel number (weight gradient)."""
        B, H, W, Cin, Cout, k, s, p = self.geom
        Ho, Wo = out_hw(self.geom)
        t = self.t
        if self.kind == "xy":
            b, n, oh, ow = idx
            xp = F.pad(t["x"][b], (p, p, p, p))[:, oh * s:oh * s + k, ow * s:ow * s + k]      # [C, k, k]
            inside = F.pad(torch.ones(1, H, W), (p, p, p, p))[:, oh * s:oh * s + k, ow * s:ow * s + k].reshape(-1) > 0
            av = xp.permute(1, 2, 0).reshape(k * k, Cin)[inside].reshape(-1)
            wv = t["w"][n].permute(1, 2, 0).reshape(k * k, Cin)[inside].reshape(-1)
            group = torch.arange(k * k)[inside].repeat_interleave(Cin)
            return av, wv, torch.stack([t["b"][n], t["res_y"][b, n, oh, ow]]), group
        if self.kind == "yx":
            b, c, ih, iw = idx
            av, wv, group = [], [], []
            for kh in range(k):
                for kw in range(k):
                    oh, ow = ih + p - kh, iw + p - kw
                    if oh % s or ow % s or not (0 <= oh // s < Ho and 0 <= ow // s < Wo):
                        continue
                    av.append(t["gy"][b, :, oh // s, ow // s])
                    wv.append(t["w"][:, c, kh, kw])
                    group.append(torch.full((Cout,), kh * k + kw))
            return torch.cat(av), torch.cat(wv), torch.stack([t["bx"][c], t["res_x"][b, c, ih, iw]]), torch.cat(group)
        n, c, kh, kw = idx
        xp = F.pad(t["x"][:, c], (p, p, p, p))[:, kh:kh + s * Ho:s, kw:kw + s * Wo:s]          # [B, Ho, Wo]
        av, wv = t["gy"][:, n].reshape(-1), xp.reshape(-1)
        return av, wv, t["gw0"][n, c, kh, kw].reshape(1), torch.arange(av.numel())

    def flat_index(self, idx):
        return int(np.ravel_multi_index(idx, tuple(self.ref.shape))) if self.kind != "wgrad" else \
            int(np.ravel_multi_index(idx, tuple(self.t["w"].shape)))

    def sample_elements(self):
        """A slice of the output: the corners (border pixels, first / last channel) and interior elements."""
        if self.kind == "wgrad":
            shape = tuple(self.t["w"].shape)
        else:
            shape = tuple(self.ref.shape)
        picks = set()
        for frac in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (.5, .5, .5, .5), (.3, .7, .2, .6), (.9, .1, .6, .4)):
            picks.add(tuple(min(d - 1, int(f * (d - 1) + 0.5)) for f, d in zip(frac, shape)))
        return sorted(picks)

    def eval32_sequential(self):
        """(score, elements): the sampled elements as strictly sequential float32 sums (products rounded to float32, one
        addition per term in the natural order, then the extras), scored against float64."""
        worst = 0.0
        elems = self.sample_elements()
        ref, S = self.ref.reshape(-1), self.S.reshape(-1)
        for idx in elems:
            av, wv, extra, _ = self.terms(idx)
            prods = (av * wv).numpy().astype(np.float32)
            seq = np.concatenate([prods, extra.numpy().astype(np.float32)])
            got = float(np.cumsum(seq, dtype=np.float32)[-1]) if seq.size else 0.0       # cumsum: one addition per term
            i = self.flat_index(idx)
            if float(S[i]) == 0.0:
                worst = max(worst, 0.0 if got == 0.0 else math.inf)
            else:
                worst = max(worst, abs(got - float(ref[i])) / (UNIT * float(S[i])))
        return worst, elems

    # -- the mutations a check must catch ---------------------------------------------------------------------------------
    def mutations(self, got):
        """{name: mutated copy of ``got``}: what a subtly wrong kernel would leave.  Every one must fail the bound."""
        B, H, W, Cin, Cout, k, s, p = self.geom
        out = {}
        is_w = self.kind == "wgrad"
        shape = tuple(self.t["w"].shape) if is_w else tuple(got.shape)
        n_main = int(np.prod(shape))

        def main(t):               # the 4-d part of the result (all of it for the convolutions, gw for the weight gradient)
            return t[:n_main].view(shape) if is_w else t

        # 1. one dropped tap at one border pixel (weight gradient: one border pixel dropped from one element)
        m = got.clone()
        corner = (0, 0, 0, 0) if not is_w else (0, 0, min(p, k - 1), min(p, k - 1))
        av, wv, _, group = self.terms(corner)
        sel = group == group[0]
        main(m)[corner] -= float((av[sel].double() * wv[sel].double()).sum())
        out["dropped tap at a border pixel"] = m
        # 2. one row of a ragged last tile replaced by its neighbour (GEMM rows: pixels; weight gradient: output channels)
        m = got.clone()
        if is_w:
            main(m)[-1] = main(m)[-2] if shape[0] > 1 else main(m)[-1].roll(1, 0)
        elif shape[2] * shape[3] > 1:
            flat = main(m).view(shape[0], shape[1], -1)
            flat[-1, :, -1] = flat[-1, :, -2]
        else:
            main(m)[-1] = main(m)[-2] if shape[0] > 1 else main(m)[-1].roll(1, 0)
        out["ragged-tile row replaced by its neighbour"] = m
        # 3. one output channel's bias omitted (weight gradient: one channel of the bias gradient never written)
        m = got.clone()
        if is_w:
            m[n_main + Cout // 2] = float(self.t["gb0"][Cout // 2])
        elif self.kind == "xy":
            m[:, Cout // 2] -= self.t["b"][Cout // 2].to(m.dtype)
        else:
            m[:, Cin // 2] -= self.t["bx"][Cin // 2].to(m.dtype)
        out["one channel's bias omitted"] = m
        # 4. one split-K plane / slab left out of one element: a contiguous run of terms no longer than any plane of a kernel
        m = got.clone()
        mid = tuple(d // 2 for d in shape)
        av, wv, _, _ = self.terms(mid)
        run = max(1, min(32, av.numel() // 2))
        main(m)[mid] -= float((av[:run].double() * wv[:run].double()).sum())
        out["split-K plane left out of one element"] = m
        # 5. the accumulate (residual / beta = 1) applied twice to one element
        m = got.clone()
        acc = self.t["gw0"] if is_w else self.t["res_y"] if self.kind == "xy" else self.t["res_x"]
        main(m)[mid] += acc[mid].to(m.dtype)
        out["accumulate applied twice to one element"] = m
        return out
