"""Float64 references, per-element error scales and float32 CPU evaluations of GroupNorm (+FiLM, +SiLU, +residual) and
RMSNorm, forward and backward, for the ledger of the norm kernels (tests/test_hip_norm_ledger.py).  CPU code, no GPU.

Layout: activations are [B, P, C] (NHWC with the map flattened to P = H * W pixels), per-image rows [B, C] / [B, G],
FiLM rows ss [B, 2C] = (scale | shift).  Every function takes its operands in a dict ``t`` of tensors and evaluates in
the dtype of those tensors, so the same code gives the float64 reference and a float32 evaluation in torch's own order.

The scale S of an output follows the rule of oracle/bounds.py: the same formula evaluated with every term replaced by its
absolute value (differences become sums), so that a float32 evaluation in ANY order has an error of a few 2^-24 * S per
element.  Where a non-linear function sits between two sums the rule is applied to its first-order propagation:

  * rstd = (var + eps)^-1/2.  var is a sum of squares of d = x - mean: every term is positive (condition number 1), the
    subtraction of two float32 of a common magnitude is exact, and the error of the mean shifts every d alike, which
    changes sum d^2 by 2 * delta * sum d = 0 to first order.  So S_rstd = rstd for an x that is given exactly.  Where x is
    itself a float32 sum of partial planes with the scale S_x per element, d carries that error and
    S_rstd = rstd * (1 + sum |d| S_x / (n (var + eps))), half the relative scale of var + eps.
  * z = x A + Bc with A = rstd gamma (scale + 1), Bc = (beta - mean rstd gamma)(scale + 1) + shift:
    S_z = |x||A| + |mean||A| + |beta||scale + 1| + |shift|.  The saved coefB on its own has no |x||A| term to carry the
    error of the mean, a sum with the scale S_mean = sum |x| / n >= |mean|: S_Bc = (|beta| + S_mean rstd |gamma|)|scale + 1|
    + |shift|.
  * y = silu(z) + res: S_y = 1.1 S_z + |silu(z)| + |res| (|silu'| <= 1.0999), without SiLU S_y = S_z + |res|.
  * The kernels compute silu(z) = z / (1 + e), e = exp(-z), with the hardware exponential: e = exp2(-z * log2(e)).  The
    relative error rho of e has three parts: the constant log2(e) is rounded (relative 2^-24 of the argument), the product
    -z * log2(e) is rounded (another 2^-24 of the argument), and an absolute error dt of the argument is a relative error
    ln(2) dt of exp2, so both together give 2 |z| 2^-24; the hardware exp2 is good to one ulp = 2 * 2^-24.  Hence
    rho <= (2 |z| + 2) 2^-24.  d silu / d e = -z / (1 + e)^2 and e / (1 + e)^2 = sigma (1 - sigma), so SiLU rows add
    |z| sigma (1 - sigma) (2 |z| + 2) to S.  The gradient silu'(z) = sigma (1 + z (1 - sigma)) has d sigma / d e =
    -sigma^2, i.e. a change sigma (1 - sigma) rho of sigma, and d silu' / d sigma = 1 + z (1 - 2 sigma): its term is
    (1 + |z| |1 - 2 sigma|) sigma (1 - sigma) (2 |z| + 2).  These terms are derived, not measured.
  * The backward pass recomputes z = x A + Bc from the saved coefficients, S = |x||A| + |Bc|, and |silu''| <= 1/2:
    S_gz = S_gy (|silu'(z)| + S_z / 2 + the exponential's term).

The tolerance constant is measured on the REFERENCE, never on the kernels: tests/test_cpu_norm_bounds.py evaluates every
ledger row in float32 on the CPU in torch's own order (native_group_norm / F.normalize with autograd) and strictly
sequentially (numpy cumsum: one addition per term), scores both against float64 and asserts the worst score against
``C_NORM_REF_WORST``.  The kernels get 4 times that (another summation order), the margin of oracle/bounds.py; they are
also held under 4 times the worst of torch's order alone (see ``C_NORM_TORCH_WORST``)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.bounds import UNIT, forward_error_units, rel  # noqa: F401  (re-exported for the tests)

EPS = 1e-5
RMS_EPS = 1e-12

# Worst forward_error_units of a float32 CPU evaluation over every ledger row and output, measured by
# tests/test_cpu_norm_bounds.py and rounded up:
#   * 79.96 strictly sequential: coefA of the 64 x 64 map at Cg = 16, where the variance is one chain of 65535 additions of
#     positive terms (75.99 for coefB of the 32 x 32 offset row; rows of a few hundred terms per group score 2 ... 12);
#   * 16.24 in torch's own order: coefB of the 3 x 5 offset row (mean = 100 deviations: coefB = beta - mean * A inherits the
#     relative error of torch's rstd times |mean||A|); rows of the N(0.5, 1.7) family score 2.3 ... 3.7.
# The weakest mutation on a row named for it scores 1023.5 (divisor n - 1 on the 16 x 16 map at Cg = 32, n = 8192).
C_NORM_REF_WORST = 90.0
C_NORM = 4.0 * C_NORM_REF_WORST
# The sequential chain, which no kernel has, sets that constant.  The kernels sum in blocks - nv values per thread, then
# ppb / J, J and Cg partial sums in fixed-order chains, a few hundred additions at the most - as torch's own kernels do
# (cascade sums, Welford per chunk).  So the ledger ALSO holds every kernel score under 4 times the worst of torch's order
# alone; this second, narrower bound is measured on the CPU like the first.
C_NORM_TORCH_WORST = 20.0


def tolerance() -> float:
    """units of 2^-24 * S: four times the worst float32 reference (either order)"""
    return C_NORM


def tolerance_blocked() -> float:
    """units of 2^-24 * S: four times the worst float32 reference in torch's own (blocked) order"""
    return 4.0 * C_NORM_TORCH_WORST


def to(t, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in t.items()}


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _exp_term_silu(z):
    s = torch.sigmoid(z)
    return z.abs() * s * (1 - s) * (2 * z.abs() + 2)


def _exp_term_silu_grad(z):
    s = torch.sigmoid(z)
    return (1 + z.abs() * (1 - 2 * s).abs()) * s * (1 - s) * (2 * z.abs() + 2)


# =============================================================================================================================
# inputs
# =============================================================================================================================
def gn_inputs(geom, family="plain", seed=0):
    """geom = (B, C, H, W, G).  family "plain": x ~ N(0.5, 1.7); "offset": unit variance around a per-(image, group) offset
    of about 100 (the cancellation case); "small": x ~ N(0.02, 0.05), a variance of 2.5e-3 that eps = 1e-5 changes by 0.4 %."""
    B, C, H, W, G = geom
    P, Cg = H * W, C // G
    g = torch.Generator().manual_seed(1000 + seed)
    if family == "plain":
        x = torch.randn(B, P, C, generator=g) * 1.7 + 0.5
    elif family == "small":
        x = torch.randn(B, P, C, generator=g) * 0.05 + 0.02
    else:
        off = 100.0 * (1 + 0.2 * torch.randn(B, 1, G, 1, generator=g))
        x = (torch.randn(B, P, G, Cg, generator=g) + off).reshape(B, P, C)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": x, "gamma": 1 + 0.3 * r(C), "beta": 0.2 * r(C), "ss": 0.5 * r(B, 2 * C), "res": r(B, P, C), "gy": r(B, P, C),
            "gx0": r(B, P, C), "gg0": r(C), "gb0": r(C), "gss0": r(B, 2 * C), "add0": r(B, P, C)}


def planes_inputs(geom, splits, seed=0):
    """gn_inputs plus ``splits`` random float32 planes [splits, B, P, C] for x and for gy and a convolution bias; the
    float64 sum of the planes (+ bias) IS the reference x / gy."""
    B, C, H, W, G = geom
    t = gn_inputs(geom, "plain", seed)
    g = torch.Generator().manual_seed(5000 + seed)
    t["xp"] = torch.randn(splits, B, H * W, C, generator=g) * 1.2 + 0.3
    t["gyp"] = torch.randn(splits, B, H * W, C, generator=g)
    t["cbias"] = torch.randn(C, generator=g)
    return t


def stats_inputs(geom, parts, offset, seed=0):
    """A pre-bias float32 tensor ``pre`` (zero-mean-ish, or around an offset of 60 with a deviation of 1: mean square over
    variance = 3600), a convolution bias, and per image ``parts`` rows of (sum, sum of squares) per channel over the row's
    share of the pixels, computed in float64 and rounded to float32: [B * parts, 2, C]."""
    B, C, H, W, G = geom
    P = H * W
    t = gn_inputs(geom, "plain", seed)
    g = torch.Generator().manual_seed(7000 + seed)
    pre = torch.randn(B, P, C, generator=g) * (1.0 if offset else 1.3) + (60.0 if offset else 0.05)
    t["pre"] = pre
    t["cbias"] = 0.5 * torch.randn(C, generator=g)
    edges = [round(i * P / parts) for i in range(parts + 1)]
    rows = torch.zeros(B, parts, 2, C, dtype=torch.float64)
    for q in range(parts):
        sl = pre[:, edges[q]:edges[q + 1]].double()
        rows[:, q, 0] = sl.sum(1)
        rows[:, q, 1] = (sl * sl).sum(1)
    t["rows"] = rows.float().reshape(B * parts, 2, C)
    return t


def rms_inputs(geom, zero_pixel=False, seed=0):
    """geom = (B, C, H, W) -> x [N, C] over N = B H W pixels.  ``zero_pixel``: pixel 1 is all zero, pixel N - 2 has a norm
    of about 1e-3."""
    B, C, H, W = geom
    N = B * H * W
    g = torch.Generator().manual_seed(3000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(N, C)
    if zero_pixel:
        x[1] = 0.0
        x[N - 2] *= 1e-3 / math.sqrt(C)
    return {"x": x, "g": 1 + 0.2 * r(C), "res": r(N, C), "gy": r(N, C), "gx0": r(N, C), "rg": r(N, C), "gg0": r(C)}


# =============================================================================================================================
# GroupNorm forward
# =============================================================================================================================
def _per_channel(v, Cg):
    return v.repeat_interleave(Cg, dim=1)          # [B, G] -> [B, C]


def gn_forward(t, G, film, act, res, x=None, mut=None):
    """-> {mean, rstd [B, G]; A, Bc [B, C]; z, y [B, P, C]} in the dtype of ``t``.  ``mut``: one of the mutations of
    MUTATIONS_GN_FWD (what a subtly wrong kernel would compute)."""
    x = t["x"] if x is None else x
    B, P, C = x.shape
    Cg = C // G
    n = P * Cg
    xg = x.reshape(B, P, G, Cg)
    if mut == "one pixel dropped from one group's statistics":
        keep = torch.ones(B, P, G, 1, dtype=x.dtype)
        keep[B - 1, P - 1, G - 1] = 0
        cnt = keep.sum((1, 3)) * Cg
        mean = (xg * keep).sum((1, 3)) / cnt
        var = (((xg - mean[:, None, :, None]) ** 2) * keep).sum((1, 3)) / cnt
    elif mut == "one-pass E[x^2] - mean^2":
        mean = xg.sum((1, 3)) / n
        var = (xg * xg).sum((1, 3)) / n - mean * mean
    else:
        mean = xg.sum((1, 3)) / n
        var = ((xg - mean[:, None, :, None]) ** 2).sum((1, 3)) / (n - 1 if mut == "divisor n - 1" else n)
    rstd = 1 / torch.sqrt(var if mut == "eps dropped" else var + EPS)
    out = {"mean": mean, "rstd": rstd}
    out.update(gn_coefficients(t, mean, rstd, film, mut=mut))
    return gn_apply(t, out, x, act, res, mut=mut)


def gn_coefficients(t, mean, rstd, film, mut=None):
    C = t["gamma"].numel()
    Cg = C // mean.shape[1]
    a = _per_channel(rstd, Cg) * t["gamma"]
    bb = t["beta"] - _per_channel(mean, Cg) * a
    if film:
        sc = t["ss"][:, :C] + 1
        if mut == "FiLM scale without + 1 in one channel":
            sc = sc.clone()
            sc[:, C // 2] -= 1
        a = a * sc
        bb = bb * sc + t["ss"][:, C:]
    return {"A": a, "Bc": bb}


def gn_apply(t, out, x, act, res, mut=None):
    a, bb = out["A"], out["Bc"]
    if mut == "first channel of a group normalised with the previous group's mean":
        # channel c = Cg of group 1 takes group 0's mean: Bc = (beta - mean0 * rstd * gamma)(sc) + shift
        C, G = a.shape[1], out["mean"].shape[1]
        Cg = C // G
        bb = bb.clone()
        bb[:, Cg] += (out["mean"][:, 1] - out["mean"][:, 0]) * a[:, Cg]
    z = x * a[:, None, :] + bb[:, None, :]
    y = F.silu(z) if act else z
    if res:
        y = y + t["res"]
    out.update(z=z, y=y)
    return out


def gn_forward_scales(t, ref, G, film, act, res, x=None, Sx=None):
    """The scales of gn_forward's outputs (float64).  ``ref``: its float64 result; ``Sx``: the scale of x where x is a
    float32 sum itself (partial planes), None for an x that is given exactly."""
    t = to(t, torch.float64)
    x = (t["x"] if x is None else x).double()
    B, P, C = x.shape
    Cg = C // G
    n = P * Cg
    ax = x.abs() if Sx is None else Sx
    S_mean = ax.reshape(B, P, G, Cg).sum((1, 3)) / n
    S_rstd = ref["rstd"].clone()
    if Sx is not None:
        d = (x.reshape(B, P, G, Cg) - ref["mean"][:, None, :, None]).abs()
        S_rstd = S_rstd * (1 + (d * Sx.reshape(B, P, G, Cg)).sum((1, 3)) / n * ref["rstd"] ** 2)
    sc = (t["ss"][:, :C] + 1).abs() if film else torch.ones(B, C, dtype=torch.float64)
    shift = t["ss"][:, C:].abs() if film else torch.zeros(B, C, dtype=torch.float64)
    S_A = _per_channel(S_rstd, Cg) * t["gamma"].abs() * sc
    S_B = (t["beta"].abs() + _per_channel(S_mean, Cg) * _per_channel(S_rstd, Cg) * t["gamma"].abs()) * sc + shift
    amean = ref["mean"].abs() if Sx is None else S_mean
    S_z = ax * S_A[:, None, :] + _per_channel(amean, Cg)[:, None, :] * S_A[:, None, :] + \
        (t["beta"].abs() * sc + shift)[:, None, :]
    z = ref["z"]
    S_y = 1.1 * S_z + F.silu(z).abs() + _exp_term_silu(z) if act else S_z.clone()
    if res:
        S_y = S_y + t["res"].abs()
    return {"mean": S_mean, "rstd": S_rstd, "A": S_A, "Bc": S_B, "y": S_y}


# =============================================================================================================================
# GroupNorm backward
# =============================================================================================================================
# modes: "plain" overwrites everything; "acc" accumulates into gx and adds onto ggamma / gbeta (affine_beta = 1) and gss
# (gss_beta = 1); "deferred" = plain through the batched row reducer; "add" = plain, and add_out += gy
def gn_backward(t, sv, G, film, act, mode="plain", gy=None, scales=False, Sgy=None):
    """The backward pass from the saved (mean, rstd, A, Bc) ``sv``, in the dtype of ``t``:
    gz = gy silu'(z); S1 = sum_p gz, S2 = sum_p gz xhat; w = gamma (scale + 1); m1, m2 = group means of w S1, w S2;
    gx = rstd (w gz - m1 - xhat m2); ggamma = sum_b (scale + 1) S2, gbeta = sum_b (scale + 1) S1;
    gscale = gamma S2 + beta S1, gshift = S1.  ``scales``: the same with every term replaced by its absolute value."""
    ab = (lambda v: v.abs()) if scales else (lambda v: v)
    x = t["x"]
    gy = t["gy"] if gy is None else gy
    B, P, C = x.shape
    Cg = C // G
    n = P * Cg
    mean_c, rstd_c = _per_channel(sv["mean"], Cg), _per_channel(sv["rstd"], Cg)
    if scales:
        xhat = (x.abs() + mean_c.abs()[:, None, :]) * rstd_c[:, None, :]
        gz = gy.abs() if Sgy is None else Sgy
        if act:
            z = x * sv["A"][:, None, :] + sv["Bc"][:, None, :]
            S_z = x.abs() * sv["A"].abs()[:, None, :] + sv["Bc"].abs()[:, None, :]
            gz = gz * (_silu_grad(z).abs() + 0.5 * S_z + _exp_term_silu_grad(z))
    else:
        xhat = (x - mean_c[:, None, :]) * rstd_c[:, None, :]
        gz = gy
        if act:
            gz = gz * _silu_grad(x * sv["A"][:, None, :] + sv["Bc"][:, None, :])
    S1, S2 = gz.sum(1), (gz * xhat).sum(1)
    sc = t["ss"][:, :C] + 1 if film else torch.ones(B, C, dtype=x.dtype)
    w = ab(t["gamma"] * sc)
    m1 = _per_channel((w * S1).reshape(B, G, Cg).sum(2) / n, Cg)
    m2 = _per_channel((w * S2).reshape(B, G, Cg).sum(2) / n, Cg)
    if scales:
        gx = rstd_c[:, None, :] * (w[:, None, :] * gz + m1[:, None, :] + xhat * m2[:, None, :])
    else:
        gx = rstd_c[:, None, :] * (w[:, None, :] * gz - m1[:, None, :] - xhat * m2[:, None, :])
    out = {"gx": gx, "ggamma": (ab(sc) * S2).sum(0), "gbeta": (ab(sc) * S1).sum(0)}
    if film:
        out["gss"] = torch.cat([ab(t["gamma"]) * S2 + ab(t["beta"]) * S1, S1], dim=1)
    if mode == "acc":
        out["gx"] = out["gx"] + ab(t["gx0"])
        out["ggamma"] = out["ggamma"] + ab(t["gg0"])
        out["gbeta"] = out["gbeta"] + ab(t["gb0"])
        if film:
            out["gss"] = out["gss"] + ab(t["gss0"])
    if mode == "add":
        out["add"] = ab(t["add0"]) + (ab(gy) if Sgy is None or not scales else Sgy)
    return out


def gn_autograd64(t, G, film, act, res):
    """float64 autograd of F.group_norm: the textbook definition gn_forward / gn_backward must agree with."""
    d = to(t, torch.float64)
    x = d["x"].permute(0, 2, 1).clone().requires_grad_(True)         # [B, C, P]
    gamma, beta, ss = (d[k].clone().requires_grad_(True) for k in ("gamma", "beta", "ss"))
    C = gamma.numel()
    z = F.group_norm(x, G, gamma, beta, EPS)
    if film:
        z = z * (ss[:, :C, None] + 1) + ss[:, C:, None]
    y = F.silu(z) if act else z
    if res:
        y = y + d["res"].permute(0, 2, 1)
    y.backward(d["gy"].permute(0, 2, 1))
    out = {"y": y.detach().permute(0, 2, 1), "gx": x.grad.permute(0, 2, 1), "ggamma": gamma.grad, "gbeta": beta.grad}
    if film:
        out["gss"] = ss.grad
    return out


# ---- float32 in torch's own order ------------------------------------------------------------------------------------------
def gn_torch32(t, G, film, act, res, mode):
    """(forward outputs, backward outputs) in float32 through torch's own kernels: native_group_norm for y, mean, rstd;
    autograd for the gradients; the accumulate forms add the previous values in float32."""
    x = t["x"].permute(0, 2, 1).contiguous().requires_grad_(True)
    B, C, P = x.shape
    gamma, beta, ss = (t[k].clone().requires_grad_(True) for k in ("gamma", "beta", "ss"))
    zn, mean, rstd = torch.native_group_norm(x, gamma, beta, B, C, P, G, EPS)
    z = zn
    if film:
        z = z * (ss[:, :C, None] + 1) + ss[:, C:, None]
    y = F.silu(z) if act else z
    if res:
        y = y + t["res"].permute(0, 2, 1)
    y.backward(t["gy"].permute(0, 2, 1))
    fwd = {"mean": mean.detach().reshape(B, G), "rstd": rstd.detach().reshape(B, G), "y": y.detach().permute(0, 2, 1)}
    fwd.update(gn_coefficients(t, fwd["mean"], fwd["rstd"], film))
    bwd = {"gx": x.grad.permute(0, 2, 1), "ggamma": gamma.grad, "gbeta": beta.grad}
    if film:
        bwd["gss"] = ss.grad
    if mode == "acc":
        bwd["gx"] = bwd["gx"] + t["gx0"]
        bwd["ggamma"] = bwd["ggamma"] + t["gg0"]
        bwd["gbeta"] = bwd["gbeta"] + t["gb0"]
        if film:
            bwd["gss"] = bwd["gss"] + t["gss0"]
    if mode == "add":
        bwd["add"] = t["add0"] + t["gy"]
    return fwd, bwd


# ---- float32, strictly sequential -------------------------------------------------------------------------------------------
def _seq_sum(a, axis):
    """float32 sum along ``axis`` with one addition per term, in index order"""
    return np.cumsum(a, axis=axis, dtype=np.float32).take(-1, axis=axis)


def gn_sequential32(t, G, film, act, res, mode, sv=None):
    """The same in float32 with every reduction strictly sequential (numpy).  The backward pass uses the saved values
    ``sv`` when given (as the kernels do), else its own forward's."""
    f = np.float32
    x = t["x"].numpy().astype(f)
    B, P, C = x.shape
    Cg = C // G
    n = f(P * Cg)
    xg = x.reshape(B, P, G, Cg).transpose(0, 2, 1, 3).reshape(B, G, P * Cg)
    mean = _seq_sum(xg, 2) / n
    d = xg - mean[:, :, None]
    rstd = (f(1) / np.sqrt(_seq_sum(d * d, 2) / n + f(EPS))).astype(f)
    tt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (("mean", mean), ("rstd", rstd))}
    fwd = dict(tt)
    fwd.update(gn_coefficients(t, tt["mean"], tt["rstd"], film))
    fwd = gn_apply(t, fwd, t["x"], act, res)
    s = sv if sv is not None else fwd
    mean_c = np.repeat(s["mean"].numpy(), Cg, 1)[:, None, :]
    rstd_c = np.repeat(s["rstd"].numpy(), Cg, 1)[:, None, :]
    gz = t["gy"].numpy().astype(f)
    if act:
        z = torch.from_numpy(x) * s["A"][:, None, :] + s["Bc"][:, None, :]
        gz = gz * _silu_grad(z).numpy()
    xhat = (x - mean_c) * rstd_c
    S1, S2 = _seq_sum(gz, 1), _seq_sum(gz * xhat, 1)
    sc = (t["ss"][:, :C] + 1).numpy() if film else np.ones((B, C), f)
    w = t["gamma"].numpy()[None, :] * sc
    m1 = np.repeat(_seq_sum((w * S1).reshape(B, G, Cg), 2) / n, Cg, 1)[:, None, :]
    m2 = np.repeat(_seq_sum((w * S2).reshape(B, G, Cg), 2) / n, Cg, 1)[:, None, :]
    gx = rstd_c * (w[:, None, :] * gz - m1 - xhat * m2)
    bwd = {"gx": gx, "ggamma": _seq_sum(sc * S2, 0), "gbeta": _seq_sum(sc * S1, 0)}
    if film:
        bwd["gss"] = np.concatenate([t["gamma"].numpy() * S2 + t["beta"].numpy() * S1, S1], 1)
    bwd = {k: torch.from_numpy(np.ascontiguousarray(v.astype(f))) for k, v in bwd.items()}
    if mode == "acc":
        bwd["gx"] = bwd["gx"] + t["gx0"]
        bwd["ggamma"] = bwd["ggamma"] + t["gg0"]
        bwd["gbeta"] = bwd["gbeta"] + t["gb0"]
        if film:
            bwd["gss"] = bwd["gss"] + t["gss0"]
    if mode == "add":
        bwd["add"] = t["add0"] + t["gy"]
    return fwd, bwd


# =============================================================================================================================
# RMSNorm: y = x / max(||x||, 1e-12) * g * sqrt(C) (+ res)
# =============================================================================================================================
# backward modes: "plain"; "acc" = gx accumulated, the residual branch's gradient rg added, gg on top of gg0 (beta = 1);
# "deferred" = plain through the batched row reducer
def rms_forward(t, res, mut=None):
    x = t["x"]
    C = x.shape[1]
    nrm = torch.sqrt((x * x).sum(1, keepdim=True)).clamp_min(RMS_EPS)
    if mut == "one pixel takes its neighbour's norm":
        nrm = nrm.clone()
        nrm[-1] = nrm[-2]
    y = x / nrm * t["g"] * math.sqrt(C)
    return {"y": y + t["res"] if res else y}


def rms_forward_scales(t, ref, res):
    d = to(t, torch.float64)
    x = d["x"]
    nrm = torch.sqrt((x * x).sum(1, keepdim=True)).clamp_min(RMS_EPS)
    S = x.abs() / nrm * d["g"].abs() * math.sqrt(x.shape[1])
    return {"y": S + d["res"].abs() if res else S}


def rms_backward(t, mode="plain", scales=False, mut=None, ragged=0):
    """gxh = gy g sqrt(C); xh = x / n; gx = (gxh - xh <xh, gxh>) / n where ||x|| >= 1e-12, gxh / 1e-12 below the clamp
    (x / 1e-12 is linear in x there); gg = sum_pixels gy xh sqrt(C).  ``ragged``: pixels of the last, ragged pixel group
    (the mutation leaves them out of gg)."""
    ab = (lambda v: v.abs()) if scales else (lambda v: v)
    x, gy = t["x"], t["gy"]
    C = x.shape[1]
    raw = torch.sqrt((x * x).sum(1, keepdim=True))
    nrm = raw.clamp_min(RMS_EPS)
    xh = ab(x) / nrm
    gxh = ab(gy * t["g"]) * math.sqrt(C)
    dot = (xh * gxh).sum(1, keepdim=True)
    dot = torch.where(raw < RMS_EPS, torch.zeros_like(dot), dot)
    gx = (gxh + xh * dot) / nrm if scales else (gxh - xh * dot) / nrm
    contrib = ab(gy) * xh * math.sqrt(C)
    if mut == "gg without the last ragged pixel group":
        contrib = contrib[:x.shape[0] - ragged]
    gg = contrib.sum(0)
    if mode == "acc":
        gx = gx + ab(t["gx0"]) + ab(t["rg"])
        gg = gg + ab(t["gg0"])
    return {"gx": gx, "gg": gg}


def rms_torch32(t, res, mode):
    x = t["x"].clone().requires_grad_(True)
    g = t["g"].clone().requires_grad_(True)
    y = F.normalize(x, dim=1, eps=RMS_EPS) * g * math.sqrt(x.shape[1])
    if res:
        y = y + t["res"]
    y.backward(t["gy"])
    bwd = {"gx": x.grad, "gg": g.grad}
    if mode == "acc":
        bwd = {"gx": bwd["gx"] + t["gx0"] + t["rg"], "gg": bwd["gg"] + t["gg0"]}
    return {"y": y.detach()}, bwd


def rms_sequential32(t, res, mode):
    f = np.float32
    x, gy, g = (t[k].numpy().astype(f) for k in ("x", "gy", "g"))
    C = x.shape[1]
    sq = f(math.sqrt(C))
    raw = np.sqrt(_seq_sum(x * x, 1))[:, None]
    nrm = np.maximum(raw, f(RMS_EPS))
    y = x / nrm * g * sq
    if res:
        y = y + t["res"].numpy()
    xh = x / nrm
    gxh = gy * g * sq
    dot = np.where(raw < f(RMS_EPS), f(0), _seq_sum(xh * gxh, 1)[:, None])
    gx = (gxh - xh * dot) / nrm
    gg = _seq_sum(gy * xh * sq, 0)
    if mode == "acc":
        gx = gx + t["gx0"].numpy() + t["rg"].numpy()
        gg = gg + t["gg0"].numpy()
    c = lambda v: torch.from_numpy(np.ascontiguousarray(v.astype(f)))
    return {"y": c(y)}, {"gx": c(gx), "gg": c(gg)}


# =============================================================================================================================
# scoring
# =============================================================================================================================
def scores(got, ref, S):
    """{output: forward_error_units} over the outputs of ``S``"""
    return {k: forward_error_units(got[k], ref[k], S[k]) for k in S if k in got}


def worst(sc):
    return max(sc.values()) if sc else 0.0


# =============================================================================================================================
# one ledger row's operands, float64 results and scales
# =============================================================================================================================
def _round32(d, keys):
    return {k: d[k].float() for k in keys}


class GNProblem:
    """kind "gn": lgm_gn_fwd / lgm_gn_bwd on a given x.  kind "planes": x and gy are float32 partial planes whose float64
    sums (+ bias) are the reference x and gy; the forward also writes x ("xw").  kind "stats": x = pre + bias, statistics
    from float32 rows of (sum, sum of squares) of ``pre``; forward only.
    The backward pass reads the SAVED mean / rstd / A / Bc: here the float64 forward results rounded to float32, an input
    like any other, so the backward kernels are judged on their own."""

    def __init__(self, geom, family="plain", film=False, act=False, res=False, mode="plain", seed=0, kind="gn", splits=0,
                 cbias=False, parts=0, offset=False):
        self.geom, self.G, self.kind = tuple(geom), geom[4], kind
        self.film, self.act, self.res, self.mode, self.cbias = film, act, res, mode, cbias
        Sx = Sgy = gy64 = None
        if kind == "planes":
            t = planes_inputs(geom, splits, seed)
            x64 = t["xp"].double().sum(0) + (t["cbias"].double() if cbias else 0.0)
            Sx = t["xp"].double().abs().sum(0) + (t["cbias"].double().abs() if cbias else 0.0)
            gy64, Sgy = t["gyp"].double().sum(0), t["gyp"].double().abs().sum(0)
            t["x"] = x64.float()                      # what the backward pass is given
        elif kind == "stats":
            t = stats_inputs(geom, parts, offset, seed)
            t["x"] = (t["pre"].double() + (t["cbias"].double() if cbias else 0.0)).float()
            x64 = t["x"].double()
        else:
            t = gn_inputs(geom, family, seed)
            x64 = t["x"].double()
        self.t = t
        d = to(t, torch.float64)
        self.ref_f = gn_forward(d, self.G, film, act, res, x=x64)
        self.S_f = gn_forward_scales(t, self.ref_f, self.G, film, act, res, x=x64, Sx=Sx)
        if kind == "planes":
            self.ref_f["xw"], self.S_f["xw"] = x64, Sx
        self.sv = _round32(self.ref_f, ("mean", "rstd", "A", "Bc"))
        if kind != "stats":
            sv64 = to(self.sv, torch.float64)
            self.ref_b = gn_backward(d, sv64, self.G, film, act, mode, gy=gy64)
            self.S_b = gn_backward(d, sv64, self.G, film, act, mode, gy=gy64, scales=True, Sgy=Sgy)

    def plane_sum32(self, skip=None):
        """x as the float32 sum of the planes in plane order, then the bias (``skip``: one plane left out)"""
        xp = self.t["xp"]
        x = None
        for i in range(xp.shape[0]):
            if i != skip:
                x = xp[i].clone() if x is None else x + xp[i]
        return x + self.t["cbias"] if self.cbias else x

    def eval32(self, sequential):
        """(forward, backward) outputs of a float32 CPU evaluation"""
        t = dict(self.t)
        if self.kind == "planes":
            xs = self.plane_sum32()
            gys = self.t["gyp"][0].clone()
            for i in range(1, self.t["gyp"].shape[0]):
                gys = gys + self.t["gyp"][i]
            tf = dict(t, x=xs)
            f, _ = (gn_sequential32 if sequential else gn_torch32)(tf, self.G, self.film, self.act, self.res, self.mode)
            f["xw"] = xs
            tb = dict(t, gy=gys)
            if sequential:
                _, b = gn_sequential32(tb, self.G, self.film, self.act, self.res, self.mode, sv=self.sv)
            else:
                _, b = gn_torch32(tb, self.G, self.film, self.act, self.res, self.mode)
            return f, b
        if sequential:
            return gn_sequential32(t, self.G, self.film, self.act, self.res, self.mode, sv=self.sv)
        return gn_torch32(t, self.G, self.film, self.act, self.res, self.mode)

    def mutated_forward32(self, mut):
        """The float32 forward with one mutation (in torch's order of plain tensor sums)"""
        x = self.plane_sum32(skip=self.t["xp"].shape[0] - 1) if mut == "one plane left out of the plane sum" else \
            self.plane_sum32() if self.kind == "planes" else self.t["x"]
        out = gn_forward(self.t, self.G, self.film, self.act, self.res, x=x, mut=mut)
        if self.kind == "planes":
            out["xw"] = x
        return out


class RMSProblem:
    def __init__(self, geom, res=False, mode="plain", zero_pixel=False, seed=0):
        self.geom, self.res, self.mode, self.zero_pixel = tuple(geom), res, mode, zero_pixel
        self.t = rms_inputs(geom, zero_pixel, seed)
        d = to(self.t, torch.float64)
        self.ref_f, self.S_f = rms_forward(d, res), rms_forward_scales(self.t, None, res)
        self.ref_b, self.S_b = rms_backward(d, mode), rms_backward(d, mode, scales=True)

    def eval32(self, sequential):
        return (rms_sequential32 if sequential else rms_torch32)(self.t, self.res, self.mode)
