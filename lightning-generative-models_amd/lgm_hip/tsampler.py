"""Timestep samplers of the diffusion training step (``GaussianDiffusion(t_sampler=...)``).

    "uniform"             torch.randint, the reference's draw: no object of this module exists
    "stratified"          one uniform per step, t_b = floor(T (u0 + b / B mod 1)) (Kingma et al. 2021, VDM App. I.1): no state,
                          importance weight 1
    "loss_second_moment"  p_t proportional to sqrt(E[L_t^2]) over the last ``history`` losses seen at t, mixed with
                          ``uniform_prob`` of the uniform distribution, loss weighted by 1 / (T p_t) (Nichol & Dhariwal 2021, 3.3)

Everything runs on the device in two launches, ``lgm_tsampler_draw`` in front of q_sample and ``lgm_tsampler_update`` behind the
loss, so a captured training step carries the sampler inside its graph: no host read, no graph boundary.  The state tensors
(``history`` [T, H] float32, ``counts`` [T] int32) and the plan the next draw reads (``cdf``, ``iw`` [T]) are plain attributes
of this object, NOT module buffers: they stay out of the flat parameter buffer, the EMA shadow and ``ddp_buffers()``; the
diffusion writes them into its state dict itself (``t_sampler.history`` / ``t_sampler.counts``) and moves them with ``_apply``.
tests/tsampler_ref.py restates the semantics in float64.
"""
from __future__ import annotations

import torch

from . import ops

T_SAMPLERS = ("uniform", "stratified", "loss_second_moment")
MODE_STRATIFIED, MODE_CDF = 0, 1


def check_arguments(t_sampler, history, uniform_prob):
    """The constructor checks of ``GaussianDiffusion``; -> (history, uniform_prob) as int and float."""
    if t_sampler not in T_SAMPLERS:
        raise ValueError("t_sampler must be 'uniform', 'stratified' or 'loss_second_moment', got " + repr(t_sampler))
    if isinstance(history, bool) or not isinstance(history, int) or history < 1:
        raise ValueError(f"t_sampler_history must be an integer >= 1, got {history!r}")
    if isinstance(uniform_prob, bool) or not isinstance(uniform_prob, (int, float)) or not 0.0 <= float(uniform_prob) <= 1.0:
        raise ValueError(f"t_sampler_uniform_prob must lie in [0, 1], got {uniform_prob!r}")
    return int(history), float(uniform_prob)


class TimestepSampler:
    """The sampler of one ``GaussianDiffusion`` in training mode (``kind`` is not "uniform")."""

    def __init__(self, kind: str, T: int, history: int = 10, uniform_prob: float = 0.001):
        assert kind in T_SAMPLERS[1:]
        self.kind, self.T, self.H, self.q = kind, int(T), int(history), float(uniform_prob)
        self.loss_aware = kind == "loss_second_moment"
        self.history = self.counts = self.cdf = self.iw = None
        if self.loss_aware:
            self.history = torch.zeros(self.T, self.H)
            self.counts = torch.zeros(self.T, dtype=torch.int32)
            self.cdf = torch.empty(self.T)
            self.iw = torch.ones(self.T)
        self._plan_stale = self.loss_aware           # cdf / iw do not belong to the state above yet

    def tensors(self):
        return ("history", "counts", "cdf", "iw") if self.loss_aware else ()

    def apply(self, fn):
        """``nn.Module._apply`` for the tensors held here (``.to(device)``)"""
        for k in self.tensors():
            setattr(self, k, fn(getattr(self, k)))
        self._plan_stale = self.loss_aware

    # ---- state -----------------------------------------------------------------------------------------------------
    def state(self):
        return {"history": self.history, "counts": self.counts} if self.loss_aware else {}

    def load_state(self, history, counts):
        """In place (a captured graph keeps reading these tensors); the plan is rebuilt before the next draw."""
        history, counts = torch.as_tensor(history), torch.as_tensor(counts)
        if tuple(history.shape) != (self.T, self.H) or tuple(counts.shape) != (self.T,):
            raise ValueError(f"t_sampler state must be history [{self.T}, {self.H}] and counts [{self.T}], got "
                             f"{tuple(history.shape)} and {tuple(counts.shape)}")
        with torch.no_grad():
            self.history.copy_(history.to(self.history.dtype))
            self.counts.copy_(counts.to(self.counts.dtype).clamp(0, self.H))
        self._plan_stale = True

    def snapshot(self):
        return [getattr(self, k).clone() for k in self.tensors()], self._plan_stale

    def restore(self, snap):
        saved, self._plan_stale = snap
        with torch.no_grad():
            for k, s in zip(self.tensors(), saved):
                getattr(self, k).copy_(s)

    def warm_fraction(self) -> float:
        """share of the rows that are full (a host read: at log time only)"""
        return float((self.counts >= self.H).float().mean()) if self.loss_aware else 1.0

    # ---- launches --------------------------------------------------------------------------------------------------
    def ensure_plan(self):
        """cdf / iw of the state as it stands (after construction, a move or a load): the update launch with an empty batch"""
        if self._plan_stale:
            self._launch_update(None, None, 1, 0.0, 0)
            self._plan_stale = False

    def draw(self, B: int, device) -> torch.Tensor:
        """t [B] int64.  The uniforms are torch's, at the place in the draw order where ``randint`` stands for "uniform"."""
        device = torch.device(device)
        t = torch.empty(B, dtype=torch.long, device=device)
        if self.loss_aware:
            if self.cdf.device != device:
                raise RuntimeError(f"the t_sampler state is on {self.cdf.device}, the batch on {device}: move the diffusion")
            self.ensure_plan()
            u = torch.rand(B, device=device)
            ops.lib().lgm_tsampler_draw(u.data_ptr(), self.cdf.data_ptr(), self.T, MODE_CDF, t.data_ptr(), B, ops.stream())
        else:
            u = torch.rand(1, device=device)
            ops.lib().lgm_tsampler_draw(u.data_ptr(), None, self.T, MODE_STRATIFIED, t.data_ptr(), B, ops.stream())
        return t

    def record(self, t, per, n_terms: int, vb_weight: float):
        """Behind the loss: the batch's unweighted per-sample losses into the rows, then the plan of the next draw."""
        self._launch_update(t, per, n_terms, vb_weight, t.shape[0])

    def _launch_update(self, t, per, n_terms, vb_weight, B):
        ops.lib().lgm_tsampler_update(None if t is None else t.data_ptr(), None if per is None else per.data_ptr(), n_terms,
                                      float(vb_weight), self.history.data_ptr(), self.counts.data_ptr(), self.H, self.q, self.T,
                                      B, self.cdf.data_ptr(), self.iw.data_ptr(), ops.stream())
