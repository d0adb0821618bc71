"""Float64 numpy restatement of elucidated diffusion (Karras et al. 2022, Table 1 "Ours", Algorithm 2) and of the random /
learned Fourier time embedding, written from the paper and independent of lgm_hip/edm.py and csrc/edm.hip: coefficients,
target, the loss in both forms, grid, gamma, one Euler and one Heun step, the Fourier row and its weight gradient - each
with the magnitude expression M the per-element bounds of tests/test_hip_edm.py are stated in.

The bound form is tests/test_hip_distill.py's: |kernel - float64| <= (k + 2) u M with u = 2^-24, k the number of float32
roundings on the longest path to that output (DESIGN 6 derives them; ``ROUNDINGS`` below) and M the expression with
magnitudes for operands.  Coefficients that reach the kernel already rounded (a sampling row, rounded once on the host) are
taken as the float64 value of that float32: they cost no rounding in the comparison."""
import math

import numpy as np

U = 2.0 ** -24
GAMMA_MAX = math.sqrt(2.0) - 1.0

# float32 roundings on the longest path, in the kernels' order (no contraction; division and sqrt round once):
#   coefficients from a float32 sigma   s2 = s s + sd sd: 3;  r = sqrt(s2): 4;  c_in = 1 / r: 5;  c_skip = sd sd / s2: 5;
#                                       c_out = (s sd) / r: 6
#   qsample xin    = c_in (y + s eps)         5 + normalise 1 + product 1 + sum 1 + product 1          = 9
#   qsample target = (y - c_skip x) / c_out   y 1, x 3, c_skip 5, product 1, difference 1, c_out 6, quotient 1 = 18
#   pre     xhat   = x + coef eps             2;      xin = c_in xhat: 3
#   euler   x'     = xh + dt ((xh - D) / s)   D = c_skip xh + c_out F: 3; difference 1, quotient 1, product 1, sum 1   = 7
#           d 5;  xin' = c_in' x': 8
#   heun    x_next = xh + dt ((d + d') / 2)   d' 5 (from the kernel's own x'), sum 1, half exact, product 1, sum 1     = 8
#   fourier row    sin / cos(((x w) 2) pi)    argument 2 (the doubling is exact), the function 1 ulp = 2 u             = 4
#   fourier g_w    2 pi sum_b x_b (c gs - s gc)   per term 4, B - 1 sums, doubling exact, times pi 1                 = B + 4
ROUNDINGS = {"xin": 9, "target": 18, "xhat": 2, "pre_xin": 3, "euler_x": 7, "euler_d": 5, "euler_xin": 8, "heun_x": 8,
             "fourier": 4}


def coefficients(sigma, sd):
    """(c_in, c_noise, c_skip, c_out) of float64 ``sigma`` (array or scalar)"""
    sigma = np.asarray(sigma, dtype=np.float64)
    s2 = sigma ** 2 + sd ** 2
    return 1.0 / np.sqrt(s2), np.log(sigma) / 4.0, sd ** 2 / s2, sigma * sd / np.sqrt(s2)


def loss_weight(sigma, sd):
    sigma = np.asarray(sigma, dtype=np.float64)
    return (sigma ** 2 + sd ** 2) / (sigma * sd) ** 2


def col(v):
    return np.asarray(v, dtype=np.float64).reshape(-1, 1, 1, 1)


def qsample(y, eps, sigma, sd):
    """NCHW float64 -> (x, c_in x, F*, M of c_in x, M of F*)"""
    c_in, _, c_skip, c_out = (col(c) for c in coefficients(sigma, sd))
    s = col(sigma)
    x = y + s * eps
    mx = np.abs(y) + np.abs(s * eps)
    return x, c_in * x, (y - c_skip * x) / c_out, c_in * mx, (np.abs(y) + c_skip * mx) / c_out


def loss_textbook(F, y, x, sigma, sd):
    """mean_b mean_elem lambda(sigma_b) (D - y)^2 with D = c_skip x + c_out F"""
    _, _, c_skip, c_out = (col(c) for c in coefficients(sigma, sd))
    D = c_skip * x + c_out * F
    B = y.shape[0]
    return float((loss_weight(sigma, sd) * ((D - y) ** 2).reshape(B, -1).mean(1)).mean())


def loss_fspace(F, target):
    """mean_b mean_elem (F - F*)^2"""
    B = F.shape[0]
    return float(((F - target) ** 2).reshape(B, -1).mean(1).mean())


def grid(N, smin, smax, rho):
    a, b = smax ** (1.0 / rho), smin ** (1.0 / rho)
    g = [(a + i / (N - 1) * (b - a)) ** rho for i in range(N)]
    g[0], g[-1] = float(smax), float(smin)
    return g + [0.0]


def gamma(sig, N, churn, tmin, tmax):
    return min(churn / N, GAMMA_MAX) if tmin <= sig <= tmax else 0.0


def plan(N, smin, smax, sd, rho, churn=0.0, tmin=0.05, tmax=50.0, snoise=1.003):
    """rows of 16 as csrc/edm.hip reads them (include/lgm_hip.h)"""
    g = grid(N, smin, smax, rho)
    rows = []
    for i in range(N):
        gm = gamma(g[i], N, churn, tmin, tmax)
        hat = g[i] * (1.0 + gm)
        row = [g[i], hat, math.sqrt(max(hat * hat - g[i] * g[i], 0.0)) * snoise if gm > 0 else 0.0, g[i + 1]]
        row += [float(c) for c in coefficients(hat, sd)]
        row += [float(c) for c in coefficients(g[i + 1], sd)] if g[i + 1] > 0 else [0.0] * 4
        row += [g[i + 1] - hat, gm, 0.0, 0.0]
        rows.append(row)
    return rows


def pre(x, eps, row):
    """-> (xhat, xin, M of xhat, M of xin) from a row of float64 values"""
    coef, c_in = row[2], row[4]
    xh = x + coef * eps if (eps is not None and coef != 0.0) else x
    mh = np.abs(x) + (np.abs(coef * eps) if (eps is not None and coef != 0.0) else 0.0)
    return xh, c_in * xh, mh, abs(c_in) * mh


def slope(xv, F, c_skip, c_out, s, clip):
    """-> (d, D before the clamp, M of d)"""
    raw = c_skip * xv + c_out * F
    D = np.clip(raw, -1.0, 1.0) if clip else raw
    md = (np.abs(xv) + np.abs(c_skip * xv) + np.abs(c_out * F)) / s
    return (xv - D) / s, raw, md


def euler(xh, F, row, clip):
    """-> (x', d, c_in' x', raw D, M of x', M of d)"""
    d, raw, md = slope(xh, F, row[6], row[7], row[1], clip)
    xp = xh + row[12] * d
    return xp, d, row[8] * xp, raw, np.abs(xh) + abs(row[12]) * md, md


def heun(xh, xp, d, F2, row, clip):
    """-> (x_next, raw D', M of x_next)"""
    d2, raw, md2 = slope(xp, F2, row[10], row[11], row[3], clip)
    return xh + row[12] * ((d + d2) / 2.0), raw, np.abs(xh) + abs(row[12]) * (np.abs(d) + md2) / 2.0


PI32 = float(np.float32(math.pi))        # the reference multiplies a float32 tensor by math.pi: the constant rounds to float32


def fourier_row(x, w):
    """x [B], w [half] float64 -> (row [B, 2 half + 1], M): f = 2 pi x w with the float32 pi the float32 path uses; M carries
    the argument's magnitude - an error of the argument moves sin and cos by as much"""
    f = x[:, None] * w[None, :] * 2.0 * PI32
    row = np.concatenate([x[:, None], np.sin(f), np.cos(f)], axis=1)
    m = np.concatenate([np.abs(x[:, None]), np.abs(f) + 1.0, np.abs(f) + 1.0], axis=1)
    return row, m


def fourier_wgrad(emb, gemb, half):
    """from the forward's own rows (x, sin, cos) and the gradient rows -> (g_w [half], M [half])"""
    x, s, c = emb[:, :1], emb[:, 1:1 + half], emb[:, 1 + half:1 + 2 * half]
    gs, gc = gemb[:, 1:1 + half], gemb[:, 1 + half:1 + 2 * half]
    g = 2.0 * PI32 * (x * (c * gs - s * gc)).sum(0)
    m = 2.0 * PI32 * (np.abs(x) * (np.abs(c * gs) + np.abs(s * gc))).sum(0)
    return g, m
