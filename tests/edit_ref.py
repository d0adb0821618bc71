"""Float64 numpy restatements for the editing tests (tests/test_edit_host.py, tests/test_hip_edit.py): the slerp rule of
csrc/slerp.hip and the inverse and forward DDIM loops around an arbitrary ``eps_fn``.  Written from the formulas (Song et al.
2021, eq. 12 and 4.3; Shoemake 1985), not imported from lgm_hip."""
import numpy as np

LERP_SWITCH = 1e-3          # 1 - c^2 below this: the lerp branch


def slerp_cosine(a, b):
    """per sample: (a.a, b.b, a.b, c) with c = a.b / sqrt(a.a b.b) clamped to [-1, 1] (nan where a norm is 0); a, b: [B, ...]"""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    aa, bb, ab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.clip(ab / np.sqrt(aa * bb), -1.0, 1.0)
    return aa, bb, ab, c


def slerp_coefficients(a, b, lam):
    """-> (c0, c1, lerp) per sample in float64; ``lam`` as the kernel reads it (float32 values)"""
    lam = np.asarray(lam, dtype=np.float32).astype(np.float64)
    aa, bb, _, c = slerp_cosine(a, b)
    c0, c1 = 1.0 - lam, lam.copy()
    lerp = (aa == 0.0) | (bb == 0.0) | np.isnan(c)
    with np.errstate(invalid="ignore"):
        lerp |= (1.0 - c * c) < LERP_SWITCH
    for i in np.nonzero(~lerp)[0]:
        w = np.arccos(c[i])
        c0[i], c1[i] = np.sin((1.0 - lam[i]) * w) / np.sin(w), np.sin(lam[i] * w) / np.sin(w)
    return c0, c1, lerp


def slerp(a, b, lam):
    """-> (out, mag, c0, c1, lerp): out = c0 a + c1 b and mag = |c0 a| + |c1 b| in float64, broadcast per sample"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c0, c1, lerp = slerp_coefficients(a, b, lam)
    s = (len(a),) + (1,) * (a.ndim - 1)
    k0, k1 = c0.reshape(s), c1.reshape(s)
    return k0 * a + k1 * b, np.abs(k0 * a) + np.abs(k1 * b), c0, c1, lerp


def inverse_grid(T, steps):
    """g_0 < .. < g_{N-1}: the times the reference's DDIM grid (linspace(-1, T - 1, steps + 1), truncated) visits"""
    times = np.linspace(-1.0, T - 1.0, steps + 1).astype(np.float32).astype(np.int64)
    return sorted({int(t) for t in times if t >= 0})


def ddim_move(acp, x, eps, t, u):
    """one deterministic DDIM move from level t to level u (either direction; u < 0: to the clean image), float64"""
    a_t = float(acp[t])
    x0 = (x - np.sqrt(1.0 - a_t) * eps) / np.sqrt(a_t)
    if u < 0:
        return x0
    a_u = float(acp[u])
    return np.sqrt(a_u) * x0 + np.sqrt(1.0 - a_u) * eps


def ddim_inverse_loop(acp, x, pairs, eps_fn):
    """the inverse chain: for (t, u), u > t: eps = eps_fn(x, t), x <- the move to u"""
    x = np.asarray(x, dtype=np.float64)
    for t, u in pairs:
        x = ddim_move(acp, x, eps_fn(x, t), t, u)
    return x


def ddim_forward_loop(acp, x, pairs, eps_fn):
    """the sampling chain at eta 0: for (t, s), s < t (s = -1: the image): eps = eps_fn(x, t), x <- the move to s"""
    return ddim_inverse_loop(acp, x, pairs, eps_fn)


def inverse_row(acp, t, u):
    """the float64 values of the eight-float row of the pair (t, u): head(t) and (sqrt(acp_u), 0, sqrt(1 - acp_u), 0)"""
    a_t, a_u = float(acp[t]), float(acp[u])
    return (np.sqrt(a_t), -np.sqrt(1.0 - a_t), np.sqrt(1.0 / a_t), np.sqrt(1.0 / a_t - 1.0), np.sqrt(a_u), 0.0,
            np.sqrt(1.0 - a_u), 0.0)
