"""Elementwise forward-error check of the Winograd convolution family against float64 (CPU code, no GPU).

sum |a||w| of oracle/bounds.py is no valid scale for a Winograd kernel: the transforms amplify the rounding error.  The
rigorous per-element scale is the SAME algorithm evaluated on absolute values with absolute-value matrices:

    forward / input gradient   S_W = |A^T| [ sum_c (|G||g||G^T|) (.) (|B^T||d||B|) ] |A| + |bias| + |residual|
    weight gradient            S_W = |G^T| [ sum_tiles (|A||dY||A^T|) (.) (|B^T||x||B|) ] |G| + |gw0|

(the input gradient is the forward form on gy with mirrored taps and swapped channel roles, as the kernels' weight operands
are).  S_W does not change under the diagonal rescalings implementations apply to G, B and A: it depends on the
interpolation points only (F(2x2,3x3): 0, +-1, inf as csrc/winograd.hip uses them; F(4x4,3x3): 0, +-1, +-2, inf as
csrc/winograd4.hip does).  The score of an output is max_i |got_i - ref_i| / (2^-24 S_W,i) with ``ref`` the DIRECT float64
convolution; where S_W,i == 0 the output must be exactly 0; a non-finite output scores inf (bounds.forward_error_units).

The tolerance is measured on the REFERENCE, never on the kernels: tests/test_cpu_wino_bounds.py evaluates every row of the
Winograd ledger (tests/test_hip_wino_ledger.py) as a float32 Winograd in plain torch, in torch's own einsum order and with a
strictly sequential sum over the reduction (channels in phases of KC = 8 for the convolutions, tiles for the weight
gradient), and records the worst score per transform and kind in C_WINO_REF_WORST.  The kernels get four times that, for
the reason given in oracle/bounds.py: MFMA K-blocking, FMA contraction inside the transforms and split-K planes / slabs are
another order and operation count than the CPU's."""
import math

import torch
import torch.nn.functional as F

from oracle import bounds

KC = 8          # reduction channels per phase of every Winograd convolution kernel

_D = torch.float64
MATS = {
    # F(2x2, 3x3): B^T, G, A^T
    2: (torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=_D),
        torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=_D),
        torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=_D)),
    # F(4x4, 3x3)
    4: (torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                      [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=_D),
        torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                      [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=_D),
        torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=_D)),
}

# worst forward_error_units (in units of 2^-24 S_W) of the float32 CPU Winograd over every ledger row, per (transform, kind),
# measured by tests/test_cpu_wino_bounds.py and rounded up.  Measured (torch's einsum order / strictly sequential), each on a
# row of the impulse family, where S_W is tight and one rounding of a transform is a whole unit:
#   F(2x2) conv   1.51 / 1.53      F(2x2) weight gradient  1.13 / 1.13
#   F(4x4) conv   1.84 / 1.62      F(4x4) weight gradient  1.54 / 1.36
# (the plain and offset rows stay under 1.0).  The weakest mutation of any row named for it scores 113.9 (one border pixel
# dropped from one tap of the F(4x4) weight gradient over 16384 pixels); the weakest on a convolution 280 (one split-K plane
# of 16 channels left out of one element, F(4x4) on 4x4 maps).
C_WINO_REF_WORST = {(2, "conv"): 1.6, (2, "wgrad"): 1.2, (4, "conv"): 1.9, (4, "wgrad"): 1.6}


def tolerance(m: int, kind: str) -> float:
    """The kernels' bound in units of 2^-24 S_W; kind = "conv" (forward, input gradient) | "wgrad"."""
    return 4.0 * C_WINO_REF_WORST[(m, kind)]


def mats(m, dtype, absolute=False):
    return tuple((t.abs() if absolute else t).to(dtype) for t in MATS[m])


# ---- the algorithm, in any dtype ---------------------------------------------------------------------------------------
def tiles_in(x, m):
    """[B, C, H, W] -> the (m + 2)^2 input tiles [B, C, th, tw, t, t] of the map zero-padded by one pixel"""
    B, C, H, W = x.shape
    th, tw = -(-H // m), -(-W // m)
    xp = F.pad(x, (1, tw * m - W + 1, 1, th * m - H + 1))
    return xp.unfold(2, m + 2, m).unfold(3, m + 2, m)


def tiles_out(y, m):
    """[B, N, H, W] -> its m x m tiles [B, N, th, tw, m, m] (zero beyond the map)"""
    B, N, H, W = y.shape
    th, tw = -(-H // m), -(-W // m)
    yp = F.pad(y, (0, tw * m - W, 0, th * m - H))
    return yp.view(B, N, th, m, tw, m).permute(0, 1, 2, 4, 3, 5)


def untile(Y, H, W):
    B, N, th, tw, m, _ = Y.shape
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, N, th * m, tw * m)[:, :, :H, :W]


def transform_in(x, m, absolute=False):
    Bt = mats(m, x.dtype, absolute)[0]
    return torch.einsum("ik,bcxykl,jl->bcxyij", Bt, tiles_in(x, m), Bt)


def transform_w(w, m, absolute=False):
    G = mats(m, w.dtype, absolute)[1]
    return torch.einsum("ik,nckl,jl->ncij", G, w, G)


def transform_out(M, m, absolute=False):
    At = mats(m, M.dtype, absolute)[2]
    return torch.einsum("pi,bnxyij,qj->bnxypq", At, M, At)


def conv(x, w, m, absolute=False, sequential=False, drop=None):
    """Y = A^T [ sum_c (G g G^T) (.) (B^T d B) ] A of x [B, C, H, W] with w [N, C, 3, 3] (stride 1, pad 1).
    ``sequential``: one addition per channel, in channel order (phases of KC channels one after the other).
    ``drop`` = (b, tx, ty, i, j, phase): that transform-domain point of that tile is left out of that phase."""
    V, U = transform_in(x, m, absolute), transform_w(w, m, absolute)
    if sequential:
        M = torch.zeros((x.shape[0], w.shape[0]) + tuple(V.shape[2:]), dtype=x.dtype)
        for c in range(x.shape[1]):
            M = M + V[:, c, None] * U[None, :, c, None, None]
    else:
        M = torch.einsum("bcxyij,ncij->bnxyij", V, U)
    if drop is not None:
        b, tx, ty, i, j, ph = drop
        cs = slice(ph * KC, (ph + 1) * KC)
        M = M.clone()
        M[b, :, tx, ty, i, j] -= torch.einsum("c,nc->n", V[b, cs, tx, ty, i, j], U[:, cs, i, j])
    return untile(transform_out(M, m, absolute), x.shape[2], x.shape[3])


def mirrored(w):
    """the forward-form weights of the input gradient: taps mirrored, channel roles swapped"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def wgrad(gy, x, m, absolute=False, sequential=False, drop=None):
    """gw = G^T [ sum_tiles (A dY A^T) (.) (B^T x B) ] G of gy [B, N, H, W] and x [B, C, H, W] -> [N, C, 3, 3].
    ``sequential``: one addition per tile, images / tile rows / tile columns in order.
    ``drop`` = (b, tx, ty, i, j): that transform-domain point of that tile is left out of the sum."""
    Bt, G, At = mats(m, x.dtype, absolute)
    V = transform_in(x, m, absolute)
    dM = torch.einsum("pi,bnxypq,qj->bnxyij", At, tiles_out(gy, m), At)
    if sequential:
        dU = torch.zeros(gy.shape[1], x.shape[1], m + 2, m + 2, dtype=x.dtype)
        B, _, th, tw = V.shape[:4]
        for b in range(B):
            for tx in range(th):
                for ty in range(tw):
                    dU = dU + dM[b, :, tx, ty, None] * V[b, None, :, tx, ty]
    else:
        dU = torch.einsum("bnxyij,bcxyij->ncij", dM, V)
    if drop is not None:
        b, tx, ty, i, j = drop
        dU = dU.clone()
        dU[:, :, i, j] -= dM[b, :, tx, ty, i, j, None] * V[b, None, :, tx, ty, i, j]
    return torch.einsum("ik,ncij,jl->nckl", G, dU, G)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "offset", "one_live_image", "impulse")
LIVE_IMAGE = 1          # the image of one_live_image that is not zero (never the first: its neighbours on both sides are zero)
IMPULSE_TAP = (0, 2)    # the one non-zero tap of the impulse family: off the diagonal, so that a mirrored tap lands elsewhere


def make_inputs(geom, family="plain", seed=None, yx=False):
    """Seeded float32 operands of one 3x3 layer, geom = (B, H, W, Cin, Cout): x, w, b (over Cout), gy, bx (over Cin), the
    residuals of both directions, a previous weight / bias gradient.  ``yx``: the gathered activation operand is gy (input
    gradient), so the family shapes gy and not x."""
    B, H, W, Cin, Cout = geom
    g = torch.Generator().manual_seed(sum(geom) + 7 * FAMILIES.index(family) if seed is None else seed)
    t = {
        "x": torch.randn(B, Cin, H, W, generator=g),
        "w": torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin),
        "b": torch.randn(Cout, generator=g),
        "gy": torch.randn(B, Cout, H, W, generator=g),
        "bx": torch.randn(Cin, generator=g),
        "res_y": torch.randn(B, Cout, H, W, generator=g),
        "res_x": torch.randn(B, Cin, H, W, generator=g),
        # the previous gradients of the beta = 1 accumulate: of this gradient's own magnitude, sqrt(pixels)
        "gw0": torch.randn(Cout, Cin, 3, 3, generator=g) * math.sqrt(B * H * W),
        "gb0": torch.randn(Cout, generator=g) * math.sqrt(B * H * W),
    }
    act = "gy" if yx else "x"
    if family == "offset":
        t[act] = t[act] + 3.0
    elif family == "one_live_image":
        assert B > LIVE_IMAGE
        for k in ("x", "gy"):
            live = t[k][LIVE_IMAGE].clone()
            t[k].zero_()
            t[k][LIVE_IMAGE] = live
    elif family == "impulse":
        for k in ("x", "gy"):
            full, C = t[k], t[k].shape[1]
            t[k] = torch.zeros_like(full)
            n = 0
            for m in (2, 4):                       # tile row / column 0 and last of both transforms, and the image corners
                for r in {0, m - 1, m, H - 1}:
                    for s in {0, m - 1, m, W - 1}:
                        if r < H and s < W:
                            b, c = n % B, (5 * n + 1) % C
                            t[k][b, c, r, s] = full[b, c, r, s] + 2.0
                            n += 1
        w = torch.zeros_like(t["w"])
        w[:, :, IMPULSE_TAP[0], IMPULSE_TAP[1]] = t["w"][:, :, IMPULSE_TAP[0], IMPULSE_TAP[1]] * 3.0
        t["w"] = w
    return t


class Problem:
    """One operation of one 3x3 layer under one transform (m = 2 | 4): kind = "xy" (forward) | "yx" (input gradient) |
    "wgrad".  ``ref`` is the DIRECT float64 result, ``S`` the float64 Winograd evaluation on absolute values (+ |bias| +
    |residual|, + |gw0| with beta = 1).  The weight gradient's outputs are ``ref`` / ``S`` (gw, [N, C, 3, 3]) and ``ref_b`` /
    ``S_b`` (the fused bias gradient, scored in units of 2^-24 sum |gy| under bounds.tolerance(n))."""

    def __init__(self, kind, m, geom, family="plain", bias=False, res=False, beta=0.0, seed=None):
        self.kind, self.m, self.geom, self.family, self.seed = kind, m, tuple(geom), family, seed
        self.bias, self.res, self.beta = bool(bias), bool(res), float(beta)
        if family == "one_live_image":
            assert not bias and not res, "one_live_image runs without bias and residual: the zero images must stay zero"
        self.t = make_inputs(geom, family, seed, yx=(kind == "yx"))
        d = {k: v.double() for k, v in self.t.items()}
        a = {k: v.abs() for k, v in d.items()}
        B, H, W, Cin, Cout = self.geom
        if kind == "wgrad":
            self.ref = torch.nn.grad.conv2d_weight(d["x"], (Cout, Cin, 3, 3), d["gy"], padding=1)
            self.S = wgrad(a["gy"], a["x"], m, absolute=True)
            if self.beta:
                self.ref, self.S = self.ref + self.beta * d["gw0"], self.S + abs(self.beta) * a["gw0"]
            self.ref_b, self.S_b = d["gy"].sum((0, 2, 3)), a["gy"].sum((0, 2, 3))
            if self.beta:
                self.ref_b, self.S_b = self.ref_b + self.beta * d["gb0"], self.S_b + abs(self.beta) * a["gb0"]
            self.n_bias = B * H * W
        else:
            act, w = self.operands(d)
            self.ref = F.conv2d(act, w, padding=1) + self._extras(d)
            aact, aw = self.operands(a)
            self.S = conv(aact, aw, m, absolute=True) + self._extras(a)

    # forward-form operands of the convolutions
    def operands(self, t, unmirrored=False):
        if self.kind == "xy":
            return t["x"], t["w"]
        return t["gy"], (t["w"].transpose(0, 1).contiguous() if unmirrored else mirrored(t["w"]))

    def _extras(self, t):
        b, r = ("b", "res_y") if self.kind == "xy" else ("bx", "res_x")
        out = 0.0
        if self.bias:
            out = out + t[b].view(1, -1, 1, 1)
        if self.res:
            out = out + t[r]
        return out

    @property
    def ckind(self):
        return "wgrad" if self.kind == "wgrad" else "conv"

    def tolerance(self):
        return tolerance(self.m, self.ckind)

    def eval32(self, sequential=False, nsel=None, csel=None, **mut):
        """the float32 Winograd evaluation (gw alone for the weight gradient).  ``nsel`` / ``csel``: produced / second weight
        channels to evaluate (the sequential sums are scored on a slice)."""
        t = self.t
        if self.kind == "wgrad":
            gy = t["gy"] if nsel is None else t["gy"][:, nsel]
            x = t["x"] if csel is None else t["x"][:, csel]
            gw = wgrad(gy, x, self.m, sequential=sequential, **mut)
            if self.beta:
                g0 = t["gw0"] if nsel is None else t["gw0"][nsel]
                gw = gw + self.beta * (g0 if csel is None else g0[:, csel])
            return gw
        act, w = self.operands(t, unmirrored=mut.pop("unmirrored", False))
        bname, rname = ("b", "res_y") if self.kind == "xy" else ("bx", "res_x")
        if nsel is not None:
            w = w[nsel]
        y = conv(act, w, self.m, sequential=sequential, **mut)
        if self.bias:
            y = y + (t[bname] if nsel is None else t[bname][nsel]).view(1, -1, 1, 1)
        if self.res:
            y = y + (t[rname] if nsel is None else t[rname][:, nsel])
        return y

    def score(self, got, nsel=None, csel=None):
        ref, S = self.ref, self.S
        if nsel is not None:
            ref, S = (ref[nsel], S[nsel]) if self.kind == "wgrad" else (ref[:, nsel], S[:, nsel])
        if csel is not None:
            ref, S = ref[:, csel], S[:, csel]
        return bounds.forward_error_units(got, ref, S)

    def slice_channels(self):
        """the channels the sequential sums are evaluated on: first, last and a few between, of both weight dimensions"""
        def pick(n):
            return sorted({0, 1, n // 3, n // 2, n - 2, n - 1} & set(range(n)))
        out_ch = self.ref.shape[0] if self.kind == "wgrad" else self.ref.shape[1]
        return pick(out_ch), (pick(self.ref.shape[1]) if self.kind == "wgrad" else None)

    # ---- the mutations a check must catch: what a subtly wrong kernel would leave -------------------------------------------
    def mutations(self, got, multi_image=False, planes=False):
        """{name: mutated copy of ``got``} for the float32 evaluation ``got`` of this problem's own inputs.  ``multi_image``:
        the row's unit packs several images; ``planes``: the row splits its reduction."""
        return self._wgrad_mutations(got, planes) if self.kind == "wgrad" else self._conv_mutations(got, multi_image, planes)

    def _conv_mutations(self, got, multi_image, planes):
        m, t = self.m, self.t
        act, w = self.operands(t)
        B, C, H, W = act.shape
        N = w.shape[0]
        At = mats(m, torch.float32)[2]
        out = {}
        # one tap (the centre one) dropped at one border pixel (the corner of the first image)
        g = got.clone()
        lead = int(act[0, :, 0, 0].abs().argmax())          # impulse family: the corner's one non-zero channel
        if float(w[:, lead, 1, 1].abs().max()) > 0 or self.family != "impulse":
            g[0, :, 0, 0] -= (w[:, :, 1, 1].double() @ act[0, :, 0, 0].double()).float()
            out["one tap dropped at one border pixel"] = g
        # the last output row of one tile replaced by the neighbouring tile's
        g = got.clone()
        if W >= 2 * m:
            g[0, :, m - 1, 0:m] = got[0, :, m - 1, m:2 * m]
        else:
            g[0, :, m - 1, :] = got[1, :, m - 1, :]
        out["last output row of one tile replaced by the neighbouring tile's"] = g
        # one transform-domain point of one tile left out of one 8-channel phase
        tx, ty = (H // m - 1, W // m - 1)
        out["one transform-domain point of one tile left out of one phase"] = \
            self.eval32(drop=(B - 1, tx, ty, 1, m, (C // KC) - 1))
        # one split-K plane (two phases: the shortest plane of any kernel) left out of one element
        if planes:
            g = got.clone()
            b, n, h, x_ = B // 2, N // 2, H // 2, W // 2
            part = F.conv2d(act[b:b + 1, :2 * KC].double(), w[n:n + 1, :2 * KC].double(), padding=1)
            g[b, n, h, x_] -= float(part[0, 0, h, x_])
            out["one split-K plane left out of one element"] = g
        bname, rname = ("b", "res_y") if self.kind == "xy" else ("bx", "res_x")
        if self.bias:
            g = got.clone()
            g[:, N // 2] -= t[bname][N // 2]
            out["one channel's bias omitted"] = g
        if self.res:
            g = got.clone()
            idx = (B // 2, N // 2, H // 2, W // 2)
            g[idx] += t[rname][idx]
            out["residual applied twice to one element"] = g
        if self.kind == "yx" and self.family != "one_live_image":
            out["input gradient computed with unmirrored taps"] = self.eval32(unmirrored=True)
        if multi_image:
            # the first row of image b + 1 read as the bottom padding row of image b
            b = LIVE_IMAGE - 1 if self.family == "one_live_image" else 0
            xp = F.pad(act[b:b + 1], (1, 1, 1, 1))
            xp[0, :, H + 1, 1:W + 1] = act[b + 1, :, 0, :]
            g = got.clone()
            g[b, :, H - 1, :] += (F.conv2d(xp.double(), w.double()) - F.conv2d(act[b:b + 1].double(), w.double(), padding=1))[0, :, H - 1, :].float()
            out["first row of the next image read as the bottom padding row"] = g
        # one coefficient of the output transform wrong by a factor of 2, on one output row of one tile
        V, U = transform_in(act[:1], m), transform_w(w, m)
        M = torch.einsum("cij,ncij->nij", V[0, :, 0, 0], U)
        g = got.clone()
        g[0, :, 1, 0:m] += At[1, 1] * torch.einsum("nj,qj->nq", M[:, 1, :], At)[:, :min(m, W)]
        out["one coefficient of the output transform doubled on one output row of one tile"] = g
        return out

    def _wgrad_mutations(self, got, planes):
        m, t = self.m, self.t
        B, N, H, W = t["gy"].shape
        C = t["x"].shape[1]
        G = mats(m, torch.float32)[1]
        out = {}
        g = got.clone()
        g[:, :, 1, 1] -= t["gy"][0, :, 0, 0, None] * t["x"][0, None, :, 0, 0]
        out["one border pixel dropped from one tap"] = g
        out["one transform-domain point of one tile left out"] = self.eval32(drop=(B - 1, H // m - 1, W // m - 1, 1, m))
        # one slab left out of one element: 32 pixels, the shortest chunk of any weight-gradient kernel; of the centre taps
        # of one input channel, the element that slab weighs most in (a single element's share of 32 pixels can be near 0)
        g = got.clone()
        c = C // 2
        gy0 = torch.zeros(1, N, H * W, dtype=torch.float64)
        gy0[0, :, :32] = t["gy"][0].double().reshape(N, -1)[:, :32]
        part = torch.nn.grad.conv2d_weight(t["x"][:1, c:c + 1].double(), (N, 1, 3, 3), gy0.view(1, N, H, W), padding=1)[:, 0, 1, 1]
        n = int(part.abs().argmax())
        g[n, c, 1, 1] -= float(part[n])
        out["one slab left out of one element"] = g
        if self.beta:
            g = got.clone()
            g[n, c, 2, 0] += self.beta * t["gw0"][n, c, 2, 0]
            out["beta = 1 accumulate applied twice to one element"] = g
        # one coefficient of G^T doubled on one tap row
        V = transform_in(t["x"], m)
        dM = torch.einsum("pi,bnxypq,qj->bnxyij", mats(m, torch.float32)[2], tiles_out(t["gy"], m), mats(m, torch.float32)[2])
        dU1 = torch.einsum("bnxyj,bcxyj->ncj", dM[..., 1, :], V[..., 1, :])
        g = got.clone()
        g[:, :, 1, :] += G[1, 1] * torch.einsum("ncj,jl->ncl", dU1, G)
        out["one coefficient of the output transform doubled on one tap row"] = g
        return out

    def bias_mutation(self, gb):
        """the fused bias gradient with one channel never written (beta = 0) / not accumulated"""
        g = gb.clone()
        g[g.numel() // 2] = self.beta * float(self.t["gb0"][g.numel() // 2])
        return g

    def eval32_bias(self):
        gb = self.t["gy"].sum((0, 2, 3))
        return gb + self.beta * self.t["gb0"] if self.beta else gb
