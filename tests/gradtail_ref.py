"""Float64 references and mutations of the gradient tail (csrc/optim.hip: lgm_grad_sqnorm_partial, lgm_grad_clip_scale,
lgm_adam_step_scaled, lgm_grad_accumulate).  CPU code, no GPU; the helper of tests/test_gradtail_host.py and
tests/test_hip_gradtail.py, built on oracle/streaming.py.

THE REFERENCE of a clipped update is ``oracle.streaming.adam_formula`` in float64 with ``grad_scale`` replaced by
``grad_scale * coef``; ``coef = min(1, max_norm / (norm + 1e-6))`` comes from the float64 norm of ``grad_scale * g`` - torch's
``clip_grad_norm_`` (norm type 2, error_if_nonfinite=False) applied to the gradient the optimizer would see, then torch's Adam.

THE TOLERANCE is the Adam family's: the float32 evaluation of the clipped update (float32 norm, scale rounded once to float32)
is measured against that reference by tests/test_gradtail_host.py and must stay within ``C_REF_WORST_GRADTAIL``; the
tolerance is 4 times that, as for every family of oracle/streaming.py.  Nothing here is measured against the HIP kernels."""
import math

import torch

from oracle import streaming as st

C_REF_WORST_GRADTAIL = st.C_REF_WORST_ADAM       # measured 6.17 (v, clip-coupled-n3074-step1000): the family's constant holds
CLIP_EPS = 1e-6                                   # torch.nn.utils.clip_grad_norm_'s constant

CLIP_SIZES = (5, 1027, 3074)
CLIP_CONFIGS = ("ddpm", "coupled", "adamw", "scale")
CLIP_STEPS = (1, 7, 1000)
CLIP_MAX_NORMS = (1e-3, 1.0, 1e6)
TINY_SCALE, TINY_MAX_NORM = 2.0 ** -25, 1e-6      # puts the norm of adam_inputs' gradients at 1.0e-6 ... 2.2e-6: the + 1e-6 shows

MUTATIONS = ("clip ignored", "coefficient not clamped at 1", "norm of the unscaled gradient", "+ 1e-6 left out")


def tolerance() -> float:
    return 4.0 * C_REF_WORST_GRADTAIL


def sqnorm64(g) -> float:
    """the exactly rounded sum of g^2 (every float32 square is exact in double; fsum adds without error)"""
    return math.fsum((g.detach().cpu().double() ** 2).tolist())


def norm64(g, grad_scale=1.0) -> float:
    return abs(grad_scale) * math.sqrt(sqnorm64(g))


def norm_bound(n: int) -> float:
    """relative error allowed to the float32 norm the device leaves: one rounding to float plus the summation bound"""
    return 2.0 ** -24 + n * 2.0 ** -53


def clip_scale64(g, grad_scale, max_norm, mut=None):
    """-> (grad_scale * coef, norm) as Python doubles.  NaN in g gives (NaN, NaN); an infinite norm gives coefficient 0."""
    norm = norm64(g, 1.0 if mut == "norm of the unscaled gradient" else grad_scale)
    r = max_norm / (norm + (0.0 if mut == "+ 1e-6 left out" else CLIP_EPS))
    coef = 1.0 if (r > 1.0 and mut != "coefficient not clamped at 1") else r        # NaN > 1 is false: NaN stays
    if mut == "clip ignored":
        coef = 1.0
    return grad_scale * coef, norm


def clip_scale32(g, grad_scale, max_norm):
    """the float32 evaluation: the norm of grad_scale * g by torch in float32, the coefficient from it in doubles, the scale
    rounded once to float32 -> a Python float holding a float32 value"""
    norm = float((g.float() * grad_scale).norm(2))
    r = max_norm / (norm + CLIP_EPS)
    return float(torch.tensor(grad_scale * (1.0 if r > 1.0 else r), dtype=torch.float32))


class ClipCase(st.Case):
    """One clipped Adam step from the state of ``oracle.streaming.adam_inputs``."""
    family = "adam"

    def __init__(self, n, config, step, max_norm, grad_scale=None):
        self.hp = dict(st.ADAM_CONFIGS[config])
        if grad_scale is not None:
            self.hp["grad_scale"] = grad_scale
        super().__init__(f"clip-{config}-n{n}-step{step}-max{max_norm:g}-gs{self.hp['grad_scale']:g}")
        self.n, self.config, self.step, self.max_norm = n, config, step, max_norm
        self.inputs = st.adam_inputs(n, step)
        self.scale, self.norm = clip_scale64(self.inputs[1], self.hp["grad_scale"], max_norm)
        self.ref, self.S = self._adam(self.scale, torch.float64)

    @property
    def tol(self):
        return tolerance()

    def _adam(self, scale, dtype):
        hp = dict(self.hp, grad_scale=scale)
        return st.adam_formula(*self.inputs, self.step, **hp, dtype=dtype)

    def eval32(self):
        return self._adam(clip_scale32(self.inputs[1], self.hp["grad_scale"], self.max_norm), torch.float32)[0]

    def mutation(self, name):
        """the float32 update a kernel with this deviation in its scale would leave"""
        scale, _ = clip_scale64(self.inputs[1], self.hp["grad_scale"], self.max_norm, mut=name)
        return self._adam(float(torch.tensor(scale, dtype=torch.float32)), torch.float32)[0]


def clip_cases():
    return [ClipCase(n, c, s, mx) for n in CLIP_SIZES for c in CLIP_CONFIGS for s in CLIP_STEPS for mx in CLIP_MAX_NORMS]


def mutation_cases(name):
    """the cases on which the issue names this mutation as failing"""
    if name == "clip ignored":
        return [ClipCase(n, c, s, 1.0) for n in CLIP_SIZES for c in CLIP_CONFIGS for s in CLIP_STEPS]
    if name == "coefficient not clamped at 1":
        return [ClipCase(n, "ddpm", s, 100.0) for n in CLIP_SIZES for s in CLIP_STEPS]
    if name == "norm of the unscaled gradient":
        return [ClipCase(n, "scale", s, 1.0) for n in CLIP_SIZES for s in CLIP_STEPS]
    if name == "+ 1e-6 left out":
        return [ClipCase(n, "ddpm", s, TINY_MAX_NORM, grad_scale=TINY_SCALE) for n in CLIP_SIZES for s in CLIP_STEPS]
    raise KeyError(name)


def accumulate_sum(grads):
    """the sequential float32 sum ((g1 + g2) + ...) + gK, formed by torch"""
    total = grads[0].clone()
    for g in grads[1:]:
        total = total + g
    return total
