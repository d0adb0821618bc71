"""Float64 references and forward-error bounds of the streaming kernels: the fused optimiser pass (csrc/optim.hip), the
weighted-MSE loss, colsum, and the activation / axpby / upsample / unshuffle / layout / posemb kernels at the top of
csrc/elementwise.hip (CPU code, no GPU).  The analogue of oracle/bounds.py, one section per family.

Every case carries
  ref : {name: float64 result}, written from the operation's definition (torch semantics), never from the kernel;
  S   : {name: the absolute-value companion}: the same expression with every operand and every intermediate sum replaced by
        its magnitude.  An output whose S is None is pure data movement and is compared bit for bit;
  eval32()       : the same operation in float32 on the CPU;
  mutations(got) : what a subtly wrong kernel would leave; every one must fail the bound.
Errors are counted per element in units of 2^-24 * S (bounds.forward_error_units; exact zeros where S == 0).

WHICH REFERENCE DECIDES.  Hyperparameters enter the float64 reference as the Python doubles the caller passed - torch forms
1 - beta and 1 - beta ** step in Python doubles - never rounded to float32 first.

TOLERANCES ARE MEASURED, NOT CHOSEN.  Per family C_REF_WORST_<family> is the worst score of the float32 CPU evaluation over
all of that family's cases, measured by tests/test_cpu_streaming_bounds.py and rounded up; the tolerance is 4 times that
(a kernel's contraction, expf / erff / tanhf and summation order differ from the CPU's).  Nothing here is measured against the
HIP kernels."""
import math

import numpy as np
import torch

from . import optim as OO
from .bounds import UNIT, forward_error_units  # noqa: F401  (UNIT re-exported for the tests)

# worst forward_error_units of the float32 CPU evaluation per family (tests/test_cpu_streaming_bounds.py prints them):
C_REF_WORST_ADAM = 6.5       # measured 6.17: v of the float32 formula, adam-coupled-n3074-step1000 (torch.optim.Adam itself: p 5.02)
C_REF_WORST_RMSPROP = 5.5    # measured 5.38: sq of the float32 formula, rmsprop-wd-scale-n1025
C_REF_WORST_EMA = 2.25       # measured 2.11: torch.lerp, ema-w0.0001-n3074
C_REF_WORST_COLSUM = 1.75    # measured 1.59: strictly sequential sum, colsum-300x130-beta1
C_REF_WORST_MSE = 3.25       # measured 3.16: gpre, tanh_mse-B300-C3-HW16-Cp4
C_REF_WORST_ACT = 4.0        # measured 3.70: SiLU backward with a bias, act-silu-37x64-bwd-bias
C_REF_WORST_AXPBY = 1.0      # measured 1.00: axpby-257x12-a0.5-b-2
C_REF_WORST_UPSAMPLE = 1.5   # measured 1.49: upsample2x_bwd-C12-acc
C_REF_WORST_POSEMB = 1.25    # measured 1.05: posemb-B130-dim64

C_REF_WORST = {"adam": C_REF_WORST_ADAM, "rmsprop": C_REF_WORST_RMSPROP, "ema": C_REF_WORST_EMA, "colsum": C_REF_WORST_COLSUM,
               "mse": C_REF_WORST_MSE, "act": C_REF_WORST_ACT, "axpby": C_REF_WORST_AXPBY, "upsample": C_REF_WORST_UPSAMPLE,
               "posemb": C_REF_WORST_POSEMB}

# results below the smallest normal float32 are judged absolutely: an error of 2^-126 counts as one unit there
TINY = 2.0 ** -126 / UNIT


def tolerance(family: str, n: int = None) -> float:
    """4 * C_REF_WORST_<family>; for a reduction of n terms capped by the theorem 2 * (n + splits + 2) at splits = 1, as
    bounds.tolerance does."""
    C = 4.0 * C_REF_WORST[family]
    return C if n is None else min(C, 2.0 * (n + 1 + 2))


def exact_units(got, want) -> float:
    """0.0 when ``got`` holds the bits of ``want`` (so -0.0 differs from 0.0 and NaN equals the same NaN), else inf"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (got.shape, want.shape, got.dtype)
    return 0.0 if torch.equal(got.view(torch.int32), want.view(torch.int32)) else math.inf


class Case:
    """One problem of one family.  Subclasses fill ``ref`` / ``S`` in __init__ and provide eval32() and mutations()."""
    family = ""
    n_terms = None           # reduction length, where the theorem's cap applies

    def __init__(self, name):
        self.name, self.ref, self.S = name, {}, {}

    @property
    def tol(self):
        return tolerance(self.family, self.n_terms)

    def scores(self, got):
        out = {}
        for k, r in self.ref.items():
            S = self.S.get(k)
            out[k] = exact_units(got[k], r) if S is None else forward_error_units(got[k], r, S)
        return out

    def score(self, got):
        return max(self.scores(got).values())

    def eval32(self):
        raise NotImplementedError

    def mutations(self, got):
        return {}

    def reported(self, got):
        """{name: mutated result} whose score is put on record without a verdict"""
        return {}


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _logu(g, n, lo, hi):
    return 10.0 ** (torch.rand(n, generator=g) * (hi - lo) + lo)


def _sign(g, n):
    return 1.0 - 2.0 * (torch.rand(n, generator=g) < 0.5).float()


FLAT_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 1027, 3074)     # 1024 = one workgroup of 256 x 4; 1025: a workgroup of tail only


# ---- Adam / AdamW ------------------------------------------------------------------------------------------------------------
# truth: torch.optim.Adam (coupled decay) / torch.optim.AdamW (decoupled=True); adam_formula in float64 is pinned to them by
# tests/test_cpu_streaming_bounds.py::test_adam_formula_is_torch_optim, so the formula is the reference's and not ours

ADAM_CONFIGS = {
    "ddpm": dict(lr=8e-5, betas=(0.9, 0.99), wd=0.0, decoupled=False, grad_scale=1.0),
    "default": dict(lr=1e-3, betas=(0.9, 0.999), wd=0.0, decoupled=False, grad_scale=1.0),
    "gan": dict(lr=2e-4, betas=(0.5, 0.999), wd=0.0, decoupled=False, grad_scale=1.0),
    "coupled": dict(lr=8e-5, betas=(0.9, 0.99), wd=1e-2, decoupled=False, grad_scale=1.0),
    "adamw": dict(lr=1e-3, betas=(0.9, 0.999), wd=1e-2, decoupled=True, grad_scale=1.0),
    "scale": dict(lr=8e-5, betas=(0.9, 0.99), wd=0.0, decoupled=False, grad_scale=0.125),
}
ADAM_STEPS = (1, 2, 7, 1000, 100000)       # at 100000 b ** step underflows
ADAM_EPS = 1e-8


def adam_inputs(n, step, seed=0):
    """(p, g, m, v) float32.  Gradients log-uniform over 1e-10 ... 10 with random sign and one in seven exactly 0 (eps and
    the placement of the bias correction only show when |g| reaches down to eps); parameters one third exactly 0 (exposes
    the update itself), one third ~1e-3, one third ~1; m = v = 0 at step 1, otherwise a mixed-sign m.  The last three
    elements keep a live gradient, so a tail left unchanged shows at every step."""
    g = _gen(n, step, seed, 77)
    idx = torch.arange(n)
    grad = _sign(g, n) * _logu(g, n, -10, 1)
    grad[(idx % 7 == 3) & (idx < n - 3)] = 0.0
    p = torch.randn(n, generator=g)
    p[idx % 3 == 0] = 0.0
    p[idx % 3 == 1] *= 1e-3
    if step == 1:
        return p, grad, torch.zeros(n), torch.zeros(n)
    mag = _logu(g, n, -10, 1)
    m = _sign(g, n) * mag * 0.3
    v = (mag * (0.5 + torch.rand(n, generator=g))) ** 2
    return p, grad, m, v


def adam_formula(p, g, m, v, step, lr, betas, wd, decoupled, grad_scale, eps=ADAM_EPS, dtype=torch.float64, mut=None):
    """torch's single-tensor Adam / AdamW, one step from the state (p, m, v) in ``dtype``; hyperparameters are Python
    doubles, their complements and bias corrections formed in doubles and rounded once where they meet a tensor.
    -> ({"p", "m", "v"}, {"p", "m", "v"} companions).  ``mut`` selects a deviation of section 4 of the issue."""
    b1, b2 = betas
    omb1, omb2 = 1 - b1, 1 - b2
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if mut == "complements from float32 betas":            # 1.f - b and 1.f - powf(b, step) on float arguments
        f = np.float32
        fb1, fb2 = f(b1), f(b2)
        omb1, omb2 = float(f(1) - fb1), float(f(1) - fb2)
        bc1, bc2 = float(f(1) - np.power(fb1, f(step))), float(f(1) - np.power(fb2, f(step)))
        b1, b2 = float(fb1), float(fb2)
    p0, g0, m0, v0 = (t.to(dtype) for t in (p, g, m, v))
    geff = g0 if (grad_scale == 1.0 or mut == "grad_scale ignored") else g0 * grad_scale
    S_g = g0.abs() * abs(grad_scale)
    dec = decoupled or mut == "decoupled decay where coupled is asked"
    pd = p0
    if dec:
        pd = p0 * (1 - lr * wd)
    elif wd != 0.0:
        geff = geff + p0 * wd
        S_g = S_g + wd * p0.abs()
    m1 = m0 + (geff - m0) * omb1
    v1 = v0 * b2 + geff * geff * omb2
    sq = v1.sqrt()
    if mut == "eps added before the bias-correction scaling":
        den = (sq + eps) / math.sqrt(bc2)
    elif mut == "bc2 omitted":
        den = sq + eps
    elif mut == "eps moved under the square root":
        den = (v1 / bc2 + eps * eps).sqrt()
    else:
        den = sq / math.sqrt(bc2) + eps
    delta = (lr / bc1) * ((m0 if mut == "m taken before the update" else m1) / den)
    S_m = b1 * m0.abs() + omb1 * S_g
    S_v = b2 * v0 + omb2 * geff.abs() * S_g
    # m and g + wd p cancel: the update inherits m's conditioning (a plain |p| + |delta| scores the reference at 2700)
    cond = torch.where(m1 != 0, S_m / m1.abs().clamp_min(1e-300), torch.ones_like(m1))
    S_p = pd.abs() + delta.abs() * cond
    return {"p": pd - delta, "m": m1, "v": v1}, {"p": S_p, "m": S_m, "v": S_v}


def adam_torch(p, g, m, v, step, lr, betas, wd, decoupled, grad_scale, eps=ADAM_EPS, dtype=torch.float64):
    """the same step by torch.optim.Adam / AdamW (foreach=False) from the same state"""
    par = p.to(dtype).clone().requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([par], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dtype).clone(),
                      "exp_avg_sq": v.to(dtype).clone()}
    par.grad = g.to(dtype) * grad_scale
    opt.step()
    st = opt.state[par]
    return {"p": par.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}


class AdamCase(Case):
    family = "adam"

    def __init__(self, n, config, step):
        super().__init__(f"adam-{config}-n{n}-step{step}")
        self.n, self.config, self.step, self.hp = n, config, step, ADAM_CONFIGS[config]
        self.inputs = adam_inputs(n, step)
        self.ref, self.S = adam_formula(*self.inputs, step, **self.hp)

    def eval32(self):
        return adam_formula(*self.inputs, self.step, **self.hp, dtype=torch.float32)[0]

    def eval32_torch(self):
        return adam_torch(*self.inputs, self.step, **self.hp, dtype=torch.float32)

    def _mut(self, name):
        return adam_formula(*self.inputs, self.step, **self.hp, dtype=torch.float32, mut=name)[0]

    def mutations(self, got):
        n, hp, out = self.n, self.hp, {}
        b2 = hp["betas"][1]
        wide = n >= 1023                  # deviations that show only where sqrt(v) reaches down to eps need many elements
        if float(np.float32(1 - b2 ** self.step)) != 1.0:
            out["bc2 omitted"] = self._mut("bc2 omitted")
            if wide:
                out["eps added before the bias-correction scaling"] = self._mut("eps added before the bias-correction scaling")
        if wide:
            out["eps moved under the square root"] = self._mut("eps moved under the square root")
        if b2 == 0.999:
            out["complements from float32 betas"] = self._mut("complements from float32 betas")
        if hp["wd"] != 0.0 and not hp["decoupled"]:
            out["decoupled decay where coupled is asked"] = self._mut("decoupled decay where coupled is asked")
        if hp["grad_scale"] != 1.0:
            out["grad_scale ignored"] = self._mut("grad_scale ignored")
        if n % 4:
            m = {k: t.clone() for k, t in got.items()}
            for k, old in zip(("p", "m", "v"), (self.inputs[0], self.inputs[2], self.inputs[3])):
                m[k][n - n % 4:] = old[n - n % 4:]
            out["the last n % 4 elements left unchanged"] = m
        out["m taken before the update"] = self._mut("m taken before the update")
        return out

    def reported(self, got):
        if self.hp["betas"][1] != 0.999:
            return {"complements from float32 betas": self._mut("complements from float32 betas")}
        return {}


def adam_cases():
    cases = [AdamCase(n, "ddpm", 2) for n in FLAT_SIZES if n not in (1027, 3074)]
    cases += [AdamCase(n, c, s) for n in (1027, 3074) for c in ADAM_CONFIGS for s in ADAM_STEPS]
    return cases


# ---- RMSprop -----------------------------------------------------------------------------------------------------------------
RMSPROP_CONFIGS = {"plain": dict(lr=5e-5, alpha=0.99, wd=0.0, grad_scale=1.0),
                   "wd-scale": dict(lr=5e-5, alpha=0.99, wd=1e-2, grad_scale=0.125)}


def rmsprop_formula(p, g, sq, lr, alpha, wd, grad_scale, eps=ADAM_EPS, dtype=torch.float64, mut=None):
    """torch.optim.RMSprop with its defaults (momentum 0, not centred) -> (results, companions)"""
    oma = 1 - alpha
    if mut == "complement from float32 alpha":
        oma, alpha = float(np.float32(1) - np.float32(alpha)), float(np.float32(alpha))
    p0, g0, s0 = (t.to(dtype) for t in (p, g, sq))
    geff = g0 if (grad_scale == 1.0 or mut == "grad_scale ignored") else g0 * grad_scale
    S_g = g0.abs() * abs(grad_scale)
    if wd != 0.0:
        geff = geff + p0 * wd
        S_g = S_g + wd * p0.abs()
    s1 = s0 * alpha + geff * geff * oma
    delta = lr * (geff / (s1.sqrt() + eps))
    cond = torch.where(geff != 0, S_g / geff.abs().clamp_min(1e-300), torch.ones_like(geff))
    return {"p": p0 - delta, "sq": s1}, {"p": p0.abs() + delta.abs() * cond, "sq": s0 * alpha + oma * geff.abs() * S_g}


def rmsprop_torch(p, g, sq, lr, alpha, wd, grad_scale, eps=ADAM_EPS, dtype=torch.float64):
    par = p.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.RMSprop([par], lr=lr, alpha=alpha, eps=eps, weight_decay=wd, foreach=False)
    opt.state[par] = {"step": torch.tensor(3.0), "square_avg": sq.to(dtype).clone()}
    par.grad = g.to(dtype) * grad_scale
    opt.step()
    return {"p": par.detach(), "sq": opt.state[par]["square_avg"]}


class RmspropCase(Case):
    family = "rmsprop"

    def __init__(self, n, config):
        super().__init__(f"rmsprop-{config}-n{n}")
        self.n, self.hp = n, RMSPROP_CONFIGS[config]
        p, g, _, v = adam_inputs(n, 5, seed=1)
        self.inputs = (p, g, v)
        self.ref, self.S = rmsprop_formula(*self.inputs, **self.hp)

    def eval32(self):
        return rmsprop_formula(*self.inputs, **self.hp, dtype=torch.float32)[0]

    def eval32_torch(self):
        return rmsprop_torch(*self.inputs, **self.hp, dtype=torch.float32)

    def mutations(self, got):
        n, out = self.n, {}
        if self.hp["grad_scale"] != 1.0:
            out["grad_scale ignored"] = rmsprop_formula(*self.inputs, **self.hp, dtype=torch.float32, mut="grad_scale ignored")[0]
        if n % 4:
            m = {k: t.clone() for k, t in got.items()}
            m["p"][n - n % 4:] = self.inputs[0][n - n % 4:]
            m["sq"][n - n % 4:] = self.inputs[2][n - n % 4:]
            out["the last n % 4 elements left unchanged"] = m
        return out

    def reported(self, got):
        return {"complement from float32 alpha": rmsprop_formula(*self.inputs, **self.hp, dtype=torch.float32,
                                                                 mut="complement from float32 alpha")[0]}


def rmsprop_cases():
    return [RmspropCase(n, c) for n in FLAT_SIZES for c in RMSPROP_CONFIGS]


# ---- EMA ---------------------------------------------------------------------------------------------------------------------
EMA_WEIGHTS = (0.0, 1e-4, 0.25, 0.5, 1.0)


def ema_inputs(n, seed=0):
    """(shadow, online): a quarter of the elements with an online value 1e-4 of the shadow, a quarter with a shadow 1e6 times
    the online value, a quarter the other way, and both zeros' signs among them"""
    g = _gen(n, seed, 5)
    sh, on = torch.randn(n, generator=g), torch.randn(n, generator=g)
    idx = torch.arange(n)
    on[idx % 4 == 0] *= 1e-4
    sh[idx % 4 == 1] *= 1e6
    on[idx % 4 == 2] *= 1e6
    sh[idx % 16 == 3] = -0.0
    on[idx % 16 == 7] = -0.0
    on[idx % 16 == 11] = 0.0
    return sh, on


class EmaCase(Case):
    """oracle/optim.py:ema_apply: w == 1 is the reference's "copy" (online, bit for bit), w == 0 keeps the shadow's bits"""
    family = "ema"

    def __init__(self, n, w):
        super().__init__(f"ema-w{w:g}-n{n}")
        self.n, self.w = n, w
        self.inputs = sh, on = ema_inputs(n)
        if w == 1.0:
            self.ref["shadow"], self.S["shadow"] = OO.ema_apply(sh, on, "copy", None), None
        elif w == 0.0:
            self.ref["shadow"], self.S["shadow"] = OO.ema_apply(sh, on, "skip", None).clone(), None
        else:
            self.ref["shadow"] = OO.ema_apply(sh.double(), on.double(), "lerp", w)
            self.S["shadow"] = sh.double().abs() + w * (on.double().abs() + sh.double().abs())

    def eval32(self):
        sh, on = self.inputs
        if self.w == 1.0:
            return {"shadow": on.clone()}
        if self.w == 0.0:
            return {"shadow": sh.clone()}
        return {"shadow": torch.lerp(sh, on, self.w)}

    def mutations(self, got):
        sh, on = self.inputs
        if self.w == 1.0:
            return {"s + (o - s) * 1 in place of a copy": {"shadow": sh + (on - sh) * 1.0}}
        return {}


def ema_cases():
    return [EmaCase(n, w) for n in FLAT_SIZES for w in EMA_WEIGHTS]


# ---- colsum ------------------------------------------------------------------------------------------------------------------
COLSUM_SHAPES = ((1, 4), (63, 3), (64, 5), (65, 64), (200, 65), (300, 130), (8193, 8), (16389, 4))
COLSUM_BETAS = (0.0, 1.0, 0.5)


def colsum_rows_per_block(rows):
    """the kernel's split of the rows (documented in csrc/elementwise.hip): at least 64 rows per block, at most 128 blocks"""
    r = max((rows + 127) // 128, 64)
    return (r + 3) // 4 * 4


class ColsumCase(Case):
    """out[c] = beta * out[c] + sum_r a[r, c]; beta == 0 does not read ``out`` (it may hold NaN)"""
    family = "colsum"

    def __init__(self, rows, cols, beta):
        super().__init__(f"colsum-{rows}x{cols}-beta{beta:g}")
        self.rows, self.cols, self.beta, self.n_terms = rows, cols, beta, rows + 1
        g = _gen(rows, cols, 3)
        self.a = torch.randn(rows, cols, generator=g)
        self.out0 = torch.randn(cols, generator=g) * math.sqrt(rows)
        a64 = self.a.double()
        self.ref["out"], self.S["out"] = a64.sum(0), a64.abs().sum(0)
        if beta != 0.0:
            self.ref["out"] = self.ref["out"] + beta * self.out0.double()
            self.S["out"] = self.S["out"] + abs(beta) * self.out0.double().abs()

    def _finish(self, s):
        return {"out": s if self.beta == 0.0 else s + self.beta * self.out0}

    def eval32(self):
        return self._finish(self.a.sum(0))

    def eval32_sequential(self):
        return self._finish(torch.from_numpy(np.cumsum(self.a.numpy(), axis=0, dtype=np.float32)[-1].copy()))

    def mutations(self, got):
        rows, cols, out = self.rows, self.cols, {}
        rpb = colsum_rows_per_block(rows)
        r0 = (rows - 1) // rpb * rpb                       # first row of the last split
        m = got["out"].clone()
        m -= self.a[rows - 1]
        out["one row of the last split dropped"] = {"out": m}
        if cols > 1:
            m = got["out"].clone()
            m[cols - 1] = m[cols - 2]
            out["one column of the last column block taken from its neighbour"] = {"out": m}
        if self.beta == 0.0:
            out["beta = 0 computed as 0 * out"] = {"out": got["out"] + 0.0 * torch.full((cols,), float("nan"))}
        m = got["out"].clone()
        m[cols // 2] -= float(self.a[r0:, cols // 2].double().sum())
        out["one split plane left out of one column"] = {"out": m}
        return out


def colsum_cases():
    return [ColsumCase(r, c, b) for r, c in COLSUM_SHAPES for b in COLSUM_BETAS]


# ---- weighted MSE (ddpm.py:921-925) and its VQ-VAE twin tanh_mse ---------------------------------------------------------------
MSE_SHAPES = ((1, 3, 1, 4), (5, 3, 64, 4), (3, 1, 255, 4), (2, 3, 1024, 4), (2, 3, 1025, 4), (2, 3, 2049, 4), (300, 3, 16, 4),
              (3, 5, 100, 8))        # (B, C, HW, Cpad)
MSE_T = 1000
PAD_A, PAD_B = 3.0e3, -1.5e3         # finite garbage in the pad lanes c >= C of the two operands: it must not enter the loss


def _mse_operands(B, C, HW, Cpad, seed):
    g = _gen(B, C, HW, Cpad, seed)
    a, b = torch.randn(B, HW, Cpad, generator=g), torch.randn(B, HW, Cpad, generator=g)
    a[..., C:], b[..., C:] = PAD_A, PAD_B
    t = torch.randint(0, MSE_T, (B,), generator=g)
    t[-1] = MSE_T - 1
    if B > 1:
        t[0] = 0
    lw = 0.1 + 5.0 * torch.rand(MSE_T, generator=g)
    return a, b, t, lw


class MseCase(Case):
    """per_sample[b] = lw[t_b] * mean_chw (out - target)^2, loss = mean_b; gout = gloss 2 w (out - target) / (C HW B), pad
    lanes exactly 0.  Companions: (|out| + |target|) in place of the difference."""
    family = "mse"
    gloss = 0.37

    def __init__(self, B, C, HW, Cpad, weighted):
        super().__init__(f"mse-B{B}-C{C}-HW{HW}-Cp{Cpad}-{'lw' if weighted else 'plain'}")
        self.shape, self.weighted, self.n_terms = (B, C, HW, Cpad), weighted, C * HW
        self.out, self.tgt, self.t, self.lw = _mse_operands(B, C, HW, Cpad, 1)
        (self.ref["per_sample"], self.ref["loss"], self.ref["gout"]) = self._eval(torch.float64)
        (self.S["per_sample"], self.S["loss"], self.S["gout"]) = self._eval(torch.float64, absolute=True)

    def _eval(self, dtype, absolute=False, mut=None):
        B, C, HW, Cpad = self.shape
        o, g = self.out.to(dtype), self.tgt.to(dtype)
        d = (o.abs() + g.abs()) if absolute else (o - g)
        w = self.lw[self.t].to(dtype) if self.weighted else torch.ones(B, dtype=dtype)
        if mut == "weight of sample b+1":
            w = w.roll(-1)
        live = d if mut == "pad lane included" else d[..., :C]
        ssum = (live * live).sum((1, 2))
        if mut == "the pixel HW-1 counted once more":
            ssum = ssum + (d[:, HW - 1, :C] ** 2).sum(1)
        per = ssum / ((Cpad if mut == "division by Cpad * HW" else C) * HW) * w
        loss = per.mean()
        gout = torch.zeros(B, HW, Cpad, dtype=dtype)
        gout[..., :C] = self.gloss * 2.0 * w[:, None, None] * d[..., :C] / (C * HW * (1 if mut == "backward missing the 1/B" else B))
        return per, loss.reshape(1), gout

    def eval32(self, mut=None):
        return dict(zip(("per_sample", "loss", "gout"), self._eval(torch.float32, mut=mut)))

    def mutations(self, got):
        B = self.shape[0]
        names = ["pad lane included", "the pixel HW-1 counted once more", "division by Cpad * HW"]
        if B > 1:
            names.append("backward missing the 1/B")
            if self.weighted:
                names.append("weight of sample b+1")
        return {n: self.eval32(mut=n) for n in names}


class TanhMseCase(Case):
    """xh = tanh(pre) on every lane, per_sample[b] = mean_chw (xh - target)^2; backward from a given float32 xh:
    gpre = (gloss w_recon) 2 (xh - target) / (C HW B) (1 - xh^2), pad lanes exactly 0; g2 = gloss (w_recon, w_vq)"""
    family = "mse"
    gloss, w_recon, w_vq = 0.37, 1.3, 0.25

    def __init__(self, B, C, HW, Cpad):
        super().__init__(f"tanh_mse-B{B}-C{C}-HW{HW}-Cp{Cpad}")
        self.shape, self.n_terms = (B, C, HW, Cpad), C * HW
        self.pre, self.tgt, _, _ = _mse_operands(B, C, HW, Cpad, 2)
        self.pre[..., :C] *= 1.5
        self.tgt[..., :C] = self.tgt[..., :C].tanh()
        self.xh32 = torch.tanh(self.pre)                 # the backward's operand
        for k, v in self._eval(torch.float64).items():
            self.ref[k] = v
        for k, v in self._eval(torch.float64, absolute=True).items():
            self.S[k] = v

    def _eval(self, dtype, absolute=False, mut=None):
        B, C, HW, Cpad = self.shape
        xh, g = torch.tanh(self.pre.to(dtype)), self.tgt.to(dtype)
        d = (xh.abs() + g.abs()) if absolute else (xh - g)
        live = d if mut == "pad lane included" else d[..., :C]
        ssum = (live * live).sum((1, 2))
        if mut == "the pixel HW-1 counted once more":
            ssum = ssum + (d[:, HW - 1, :C] ** 2).sum(1)
        per = ssum / ((Cpad if mut == "division by Cpad * HW" else C) * HW)
        t = self.xh32.to(dtype)
        db = (t.abs() + g.abs()) if absolute else (t - g)
        gr = self.gloss * self.w_recon
        gpre = torch.zeros(B, HW, Cpad, dtype=dtype)
        tt = (1 + t * t) if absolute else (1 - t * t)
        gpre[..., :C] = (gr * 2.0 / (C * HW * (1 if mut == "backward missing the 1/B" else B)) * db * tt)[..., :C]
        g2 = torch.tensor([gr, self.gloss * self.w_vq], dtype=dtype)
        return {"xh": xh.abs() if absolute else xh, "per_sample": per, "gpre": gpre, "g2": g2.abs() if absolute else g2}

    def eval32(self, mut=None):
        return self._eval(torch.float32, mut=mut)

    def mutations(self, got):
        names = ["pad lane included", "the pixel HW-1 counted once more", "division by Cpad * HW"]
        if self.shape[0] > 1:
            names.append("backward missing the 1/B")
        return {n: self.eval32(mut=n) for n in names}


def mse_cases():
    return [MseCase(*s, weighted=w) for s in MSE_SHAPES for w in (True, False)] + [TanhMseCase(*s) for s in MSE_SHAPES]


# ---- activations ---------------------------------------------------------------------------------------------------------------
ACTS = ("silu", "gelu", "relu", "lrelu", "tanh")
ACT_SHAPES = ((1, 4), (37, 64), (257, 12))
ACT_SPECIALS = (0.0, -0.0, 1e-8, -1e-8, 1.2785, -1.2785, 20.0, -20.0, 100.0, -100.0)
SLOPE = 0.2
_R2, _RPI = math.sqrt(0.5), 1.0 / math.sqrt(2.0 * math.pi)


def act_terms(z, act):
    """(f, |f|-companion, f', |f'|-companion, |f''|) of one activation at z, in z's dtype.  The companions replace every
    term of a sum by its magnitude: SiLU' = s + z s (1 - s) crosses zero near z = -1.28, GELU's 1 + erf and tanh's 1 - t^2
    cancel; a plain relative error is unbounded there."""
    if act == "silu":
        s = torch.sigmoid(z)
        return z * s, z.abs() * s, s + z * s * (1 - s), s + z.abs() * s * (1 - s), (s * (1 - s) * (2 + z * (1 - 2 * s))).abs()
    if act == "gelu":
        e, pdf = torch.erf(z * _R2), _RPI * torch.exp(-0.5 * z * z)
        return (0.5 * z * (1 + e), 0.5 * z.abs() * (1 + e.abs()), 0.5 * (1 + e) + z * pdf, 0.5 * (1 + e.abs()) + z.abs() * pdf,
                pdf * (2 + z * z))
    if act == "relu":
        on = (z > 0).to(z.dtype)
        return z * on, z.abs() * on, on, on, torch.zeros_like(z)
    if act == "lrelu":
        k = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))       # torch: slope at z == 0
        return z * k, z.abs() * k, k, k, torch.zeros_like(z)
    t = torch.tanh(z)
    return t, t.abs(), 1 - t * t, 1 + t * t, 2 * t.abs() * (1 + t * t)


def act_inputs(rows, cols, seed=0):
    """x = randn with the special values at every third position (while they fit), bias, residual, gy, previous gx"""
    g = _gen(rows, cols, seed, 11)
    x = torch.randn(rows, cols, generator=g)
    flat = x.view(-1)
    for i, s in enumerate(ACT_SPECIALS):
        if 1 + 3 * i < flat.numel():
            flat[1 + 3 * i] = s
    bias = 0.75 * torch.randn(cols, generator=g)
    bias = bias + 0.25 * bias.sign()
    bias[cols - 1] = -2.0 * x[0, cols - 1]        # x and x + bias differ in sign there: a lost bias shows in ReLU' too
    return x, bias, torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)


class ActCase(Case):
    """y = act(x + bias) + res and gx = (acc ? gx : 0) + gy act'(x + bias).  With a bias the pre-activation z = x + bias is
    one float32 addition (relative error 2^-24 whatever the implementation), which moves act(z) by |z act'(z)| 2^-24: the
    companions carry that term; without a bias z is exact and they do not.  TINY judges results below the smallest normal
    float32 absolutely (SiLU(-100) = -3.7e-42)."""
    family = "act"

    def __init__(self, act, rows, cols, direction, bias, res=False, acc=False):
        opts = "+".join(n for n, on in (("bias", bias), ("res", res), ("acc", acc)) if on) or "bare"
        super().__init__(f"act-{act}-{rows}x{cols}-{direction}-{opts}")
        self.act, self.direction, self.bias, self.res, self.acc = act, direction, bias, res, acc
        self.x, self.b, self.r, self.gy, self.gx0 = act_inputs(rows, cols)
        key = "y" if direction == "fwd" else "gx"
        self.ref[key], self.S[key] = self._eval(torch.float64), self._eval(torch.float64, absolute=True)

    def _eval(self, dtype, absolute=False, mut=None):
        x, b, r, gy, gx0 = (t.to(dtype) for t in (self.x, self.b, self.r, self.gy, self.gx0))
        z = x + b if self.bias else x
        if mut == "bias omitted in one four-channel group":
            z = z.clone()
            c0 = (x.shape[1] // 4 - 1) * 4
            z[:, c0:c0 + 4] = x[:, c0:c0 + 4]
        if mut == "residual added before the activation":
            z = z + r
        f, fa, d, da, d2 = act_terms(z, self.act)
        if self.direction == "fwd":
            if absolute:
                return fa + (z.abs() * da if self.bias else 0) + (r.abs() if self.res else 0) + TINY * (fa != 0)
            return f + r if (self.res and mut != "residual added before the activation") else f
        if absolute:
            return (gx0.abs() if self.acc else 0) + gy.abs() * (da + (z.abs() * d2 if self.bias else 0)) + TINY * (da != 0)
        if mut == "SiLU' without the x s (1 - s) term on one element":
            i = self._silu_element()
            d = d.clone()
            d.view(-1)[i] = torch.sigmoid(z.view(-1)[i])
        out = gy * d
        return out + gx0 if (self.acc and mut != "accumulate overwriting") else out

    def _silu_element(self):
        hit = (self.x.view(-1) == -1.2785).nonzero()
        return int(hit[0]) if hit.numel() else 0

    def eval32(self, mut=None):
        return {"y" if self.direction == "fwd" else "gx": self._eval(torch.float32, mut=mut)}

    def mutations(self, got):
        names = []
        if self.bias:
            names.append("bias omitted in one four-channel group")
        if self.direction == "fwd" and self.res:
            names.append("residual added before the activation")
        if self.direction == "bwd" and self.act == "silu":
            names.append("SiLU' without the x s (1 - s) term on one element")
        if self.direction == "bwd" and self.acc:
            names.append("accumulate overwriting")
        return {n: self.eval32(mut=n) for n in names}


def act_cases(acts=ACTS, shapes=ACT_SHAPES):
    out = []
    for act in acts:
        for rows, cols in shapes:
            for bias in (False, True):
                out += [ActCase(act, rows, cols, "fwd", bias, res=res) for res in (False, True)]
                out += [ActCase(act, rows, cols, "bwd", bias, acc=acc) for acc in (False, True)]
    return out


# ---- axpby, upsample2x_bwd, pixel-unshuffle accumulate, posemb -------------------------------------------------------------
AXPBY_COEFFS = ((1.0, 1.0), (0.5, -2.0), (0.0, 1.0))


class AxpbyCase(Case):
    """y = alpha a + beta b (b optional)"""
    family = "axpby"

    def __init__(self, rows, cols, alpha, beta, with_b):
        super().__init__(f"axpby-{rows}x{cols}-a{alpha:g}-b{beta:g}{'' if with_b else '-nob'}")
        self.alpha, self.beta, self.with_b = alpha, beta, with_b
        x, _, r, _, _ = act_inputs(rows, cols, seed=2)
        self.a, self.b = x, r
        self.ref["y"], self.S["y"] = self._eval(torch.float64), self._eval(torch.float64, absolute=True)

    def _eval(self, dtype, absolute=False, swapped=False):
        a, b = self.a.to(dtype), self.b.to(dtype)
        al, be = (self.beta, self.alpha) if swapped else (self.alpha, self.beta)
        if absolute:
            a, b, al, be = a.abs(), b.abs(), abs(al), abs(be)
        return a * al + b * be if self.with_b else a * al

    def eval32(self):
        return {"y": self._eval(torch.float32)}

    def mutations(self, got):
        return {"alpha and beta swapped": {"y": self._eval(torch.float32, swapped=True)}} if self.alpha != self.beta else {}


def axpby_cases():
    return [AxpbyCase(r, c, al, be, wb) for r, c in ACT_SHAPES for al, be in AXPBY_COEFFS for wb in (True, False)]


SPATIAL = dict(B=2, H=3, W=5)
SPATIAL_C = (4, 12)


def upsample2x_fwd(x):
    """NHWC nearest x2: y[b, 2h+i, 2w+j] = x[b, h, w]"""
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def pixel_unshuffle(hi):
    """NHWC "b (h p1) (w p2) c -> b h w (c p1 p2)" (ddpm.py:102)"""
    B, H2, W2, C = hi.shape
    return hi.reshape(B, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H2 // 2, W2 // 2, C * 4)


def pixel_shuffle(lo):
    """its inverse: lo [B, H, W, 4C] -> hi [B, 2H, 2W, C]"""
    B, H, W, C4 = lo.shape
    return lo.reshape(B, H, W, C4 // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, C4 // 4)


def nchw_to_nhwc(src, Cpad):
    """[B, C, H, W] -> [B, H*W, Cpad], pad channels exactly 0"""
    B, C, H, W = src.shape
    out = torch.zeros(B, H * W, Cpad, dtype=src.dtype)
    out[..., :C] = src.reshape(B, C, H * W).permute(0, 2, 1)
    return out


class UpsampleBwdCase(Case):
    """gx[b, h, w] = (acc ? gx : 0) + the four children of gy in the fixed order (a + b) + (c + d)"""
    family = "upsample"

    def __init__(self, C, acc):
        super().__init__(f"upsample2x_bwd-C{C}{'-acc' if acc else ''}")
        B, H, W = SPATIAL["B"], SPATIAL["H"], SPATIAL["W"]
        g = _gen(C, 19)
        self.acc = acc
        self.gy, self.gx0 = torch.randn(B, 2 * H, 2 * W, C, generator=g), torch.randn(B, H, W, C, generator=g)
        self.ref["gx"], self.S["gx"] = self._eval(torch.float64), self._eval(torch.float64, absolute=True)

    def _eval(self, dtype, absolute=False, dropped=False):
        gy, gx0 = self.gy.to(dtype), self.gx0.to(dtype)
        if absolute:
            gy, gx0 = gy.abs(), gx0.abs()
        a, b, c, d = gy[:, 0::2, 0::2], gy[:, 0::2, 1::2], gy[:, 1::2, 0::2], gy[:, 1::2, 1::2]
        s = (a + b) + (c if dropped else c + d)
        return s + gx0 if self.acc else s

    def eval32(self):
        return {"gx": self._eval(torch.float32)}

    def mutations(self, got):
        return {"one child dropped": {"gx": self._eval(torch.float32, dropped=True)}}


class UnshuffleAccCase(Case):
    """pixel_unshuffle(inverse, accumulate=True): hi += shuffle(lo), one addition per element: at most one unit of |old| + |v|"""
    family = "upsample"

    def __init__(self, C):
        super().__init__(f"unshuffle-inverse-acc-C{C}")
        B, H, W = SPATIAL["B"], SPATIAL["H"], SPATIAL["W"]
        g = _gen(C, 23)
        self.lo, self.hi0 = torch.randn(B, H, W, 4 * C, generator=g), torch.randn(B, 2 * H, 2 * W, C, generator=g)
        v = pixel_shuffle(self.lo)
        self.ref["hi"], self.S["hi"] = self.hi0.double() + v.double(), self.hi0.double().abs() + v.double().abs()

    @property
    def tol(self):
        return 1.0 + 1e-9          # <= 1 unit (one rounding is at most half of one)

    def eval32(self):
        return {"hi": self.hi0 + pixel_shuffle(self.lo)}

    def mutations(self, got):
        return {"accumulate overwriting": {"hi": pixel_shuffle(self.lo)}}


def upsample_cases():
    return [UpsampleBwdCase(C, acc) for C in SPATIAL_C for acc in (False, True)] + [UnshuffleAccCase(C) for C in SPATIAL_C]


POSEMB_SHAPES = ((1, 4, 4), (3, 64, 72), (130, 64, 64))       # (B, dim, pitch)
POSEMB_THETA = 10000.0


def posemb_freqs(dim, theta=POSEMB_THETA):
    """the reference's table (ddpm.py:127-129): float32, torch's CPU exp"""
    half = dim // 2
    return torch.exp(torch.arange(half) * -(math.log(theta) / (half - 1)))


class PosembCase(Case):
    """emb[b] = cat(sin(arg), cos(arg)) with arg the FLOAT32 product float(t_b) * freq (the kernel's contract is a host
    frequency table); sin / cos themselves in float64"""
    family = "posemb"

    def __init__(self, B, dim):
        super().__init__(f"posemb-B{B}-dim{dim}")
        g = _gen(B, dim, 29)
        self.dim = dim
        self.t = torch.randint(0, 1000, (B,), generator=g)
        for i, tv in enumerate((999, 0, 1)[:B]):
            self.t[-1 - i] = tv
        self.freqs = posemb_freqs(dim)
        self.arg = self.t.float()[:, None] * self.freqs[None, :]
        a = self.arg.double()
        self.ref["emb"] = torch.cat((a.sin(), a.cos()), -1)
        self.S["emb"] = self.ref["emb"].abs()

    def eval32(self):
        return {"emb": torch.cat((self.arg.sin(), self.arg.cos()), -1)}

    def mutations(self, got):
        if int(self.t.max()) < 100:
            return {}
        a = self.t.double()[:, None] * posemb_freqs(self.dim).double().mul(1 + 2.0 ** -23)[None, :]
        return {"frequency table off by one ulp": {"emb": torch.cat((a.sin(), a.cos()), -1).float()}}


def posemb_cases():
    return [PosembCase(B, dim) for B, dim, _ in POSEMB_SHAPES]


FAMILIES = {"adam": adam_cases, "rmsprop": rmsprop_cases, "ema": ema_cases, "colsum": colsum_cases, "mse": mse_cases,
            "act": act_cases, "axpby": axpby_cases, "upsample": upsample_cases, "posemb": posemb_cases}
