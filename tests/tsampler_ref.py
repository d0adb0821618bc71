"""The timestep samplers of the diffusion training step (lgm_hip/tsampler.py, lgm_tsampler_draw / lgm_tsampler_update) restated
in numpy.  CPU code, no GPU: the helper of tests/test_tsampler_host.py and tests/test_hip_tsampler.py.

Arithmetic that the kernels COPY or that float32 determines bit for bit is restated in float32 (the stratified draw, the
search in a given float32 cdf, the per-sample loss L_b = per0 + vb_weight per1, the rows of the history).  Arithmetic the
kernels round on their own way - the plan p, cdf, iw - is restated in float64 from the same float32 history; its bound against
the kernel, 1e-4 relative, is (T - 1) 2^-24 ~ 6e-5 for a fixed-order float32 sum of T <= 1000 non-negative terms plus a few
roundings of the square root and the divides.  Nothing here is measured against the HIP kernels."""
import numpy as np

F32 = np.float32


# ---- draws -----------------------------------------------------------------------------------------------------------------
def stratified_draw(u0, B, T):
    """t [B] int64 from ONE float32 uniform: u_b = u0 + b / B (a float32 division, then a float32 add), minus 1 where >= 1."""
    u = F32(u0) + np.arange(B, dtype=F32) / F32(B)
    u = np.where(u >= F32(1), u - F32(1), u).astype(F32)
    return np.minimum(T - 1, np.floor(F32(T) * u).astype(np.int64))


def cdf_draw(cdf, u):
    """the first index with cdf[t] > u_b, T - 1 where there is none"""
    cdf, u = np.asarray(cdf, F32), np.asarray(u, F32)
    return np.minimum(len(cdf) - 1, np.searchsorted(cdf, u, side="right")).astype(np.int64)


# ---- state -----------------------------------------------------------------------------------------------------------------
class State:
    """history as one chronological list per timestep (at most H float32 values, oldest first); counts = their lengths"""

    def __init__(self, T, H, rows=None):
        self.T, self.H = int(T), int(H)
        self.rows = [[] for _ in range(T)] if rows is None else [list(map(F32, r))[-H:] for r in rows]

    @classmethod
    def from_arrays(cls, history, counts):
        history = np.asarray(history, F32)
        return cls(history.shape[0], history.shape[1], [history[t, :int(c)] for t, c in enumerate(counts)])

    @property
    def counts(self):
        return np.array([len(r) for r in self.rows], np.int32)

    def arrays(self):
        """(history [T, H] float32 with the held entries in front and zeros behind, counts [T] int32)"""
        h = np.zeros((self.T, self.H), F32)
        for t, r in enumerate(self.rows):
            h[t, :len(r)] = r
        return h, self.counts

    def warm(self):
        return all(len(r) == self.H for r in self.rows)

    def update(self, t, L):
        """in batch order: append L_b to row t_b, keep the last H; a non-finite L_b or a t_b outside [0, T) is not recorded"""
        for tb, lb in zip(np.asarray(t).tolist(), np.asarray(L, F32).tolist()):
            if 0 <= tb < self.T and np.isfinite(lb):
                self.rows[tb] = (self.rows[tb] + [F32(lb)])[-self.H:]


def per_sample_loss(per, vb_weight=None):
    """L_b in float32 as the update kernel forms it: per [B] (plain network: loss_weight[t_b] mse_b) or per [2, B] with
    L_b = per[0] + vb_weight * per[1], product and sum rounded separately"""
    per = np.asarray(per, F32)
    if per.ndim == 1:
        return per
    return (per[0] + (F32(vb_weight) * per[1]).astype(F32)).astype(F32)


# ---- plan ------------------------------------------------------------------------------------------------------------------
def plan(state, q):
    """-> (p, cdf, iw, weighted) in float64.  Not warm, or sum(w) zero (or not finite): p = 1 / T, iw = 1."""
    T, H = state.T, state.H
    uniform = np.full(T, 1.0 / T), np.ones(T)
    if not state.warm():
        p, iw, weighted = *uniform, False
    else:
        w = np.array([np.sqrt(np.mean(np.asarray(r, np.float64) ** 2)) for r in state.rows])
        tot = w.sum()
        if not (tot > 0 and np.isfinite(tot)):
            p, iw, weighted = *uniform, False
        else:
            p = (1.0 - q) * w / tot + q / T
            with np.errstate(divide="ignore"):
                iw, weighted = 1.0 / (T * p), True
    cdf = np.cumsum(p)
    cdf[-1] = 1.0
    return p, cdf, iw, weighted


def weighted_loss(iw, t, L):
    """mean_b(iw[t_b] L_b) in float64 and its derivative in L_b, iw[t_b] / B"""
    w = np.asarray(iw, np.float64)[np.asarray(t)]
    return float(np.mean(w * np.asarray(L, np.float64))), w / len(w)
