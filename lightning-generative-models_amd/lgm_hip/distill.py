"""Progressive distillation of the DDPM sampler (Salimans & Ho 2022, Algorithm 2; an extension of the reference) - the host
side: the nested time grids, the float64 coefficient rows the two kernels of csrc/distill.hip read, and the refusals.  Pure
Python and torch on the host: no device, no library.

A student with N sampling steps is trained so that ONE of its DDIM steps (eta = 0) reproduces TWO DDIM steps of a frozen
teacher.  With T = ``num_timesteps``:

    G2 = reversed(linspace(-1, T - 1, 2 N + 1).int())     the teacher's levels: ``ddim_time_pairs()`` at 2 N steps, last one -1
    G  = G2[::2]                                          the student's levels: ``ddim_time_pairs()`` at N steps

and per sample i ~ randint(0, N), t = G[i], t' = G2[2 i + 1], t'' = G[i + 1].  ``distill_grid`` refuses a (T, N) whose G is not
the grid ``ddim_sample`` walks at N steps (the truncation of linspace does not nest for every pair).

Write a_s = sqrt_alphas_cumprod[s], s_s = sqrt_one_minus_alphas_cumprod[s], a_-1 = 1, s_-1 = 0.  From z_t = a_t x + s_t eps:

    (x1, e1) = teacher's model_predictions(z_t, t)        clip_x_start = clip, rederive_pred_noise = True: what ddim_sample forms
    z_t'     = a_t' x1 + s_t' e1
    (x2, e2) = teacher's model_predictions(z_t', t')
    z_t''    = a_t'' x2 + s_t'' e2
    x~       = (z_t'' - r z_t) / (a_t'' - r a_t),  r = s_t'' / s_t            (x~ = z_t'' when t'' = -1)
    target   = x~ | e~ = (z_t - a_t x~) / s_t | a_t e~ - s_t x~               (student's pred_x0 | pred_noise | pred_v)

x~ is the x0 prediction with which one DDIM step of the student from z_t lands on z_t''.  The kernels evaluate x~ as
cX z_t'' + cZ z_t with cX = 1 / den, cZ = -r / den, den = a_t'' - r a_t: the two coefficients are formed in float64 and rounded
once, so the only cancellation left is the one of the two products (bounded per element in tests/distill_ref.py).

The schedule the rows are planned from is the diffusion's four float32 tables read as float64 - each of them is its float64
value rounded once, none is a difference of rounded values, and the heads (A, S, R, Rm1) in a row are then bit for bit the
scalars the teacher's ``ddim_sample`` reads at the same timestep."""
from __future__ import annotations

import math
from typing import List, Tuple

import torch

ROW = 16           # floats per table row (csrc/distill.hip)
(A_T, S_T, R_T, RM1_T, A_M, S_M, R_M, RM1_M, A_N, S_N, CX, CZ, IS_T, T_MID, DEN, T_NEXT) = range(ROW)


def _levels(T: int, steps: int) -> List[int]:
    """the levels ``GaussianDiffusion.ddim_time_pairs()`` walks at ``sampling_timesteps = steps``: steps + 1 entries, the last -1"""
    return list(reversed(torch.linspace(-1, T - 1, steps=steps + 1).int().tolist()))


def distill_grid(T: int, N: int) -> Tuple[List[int], List[int]]:
    """-> (G, G2): the student's N + 1 levels and the teacher's 2 N + 1.  ValueError naming (T, N) when N < 1, 2 N > T, G2 does
    not decrease strictly or G2[::2] is not the grid ``ddim_sample`` walks at N steps."""
    T, N = int(T), int(N)
    if N < 1 or 2 * N > T:
        raise ValueError(f"distillation to N steps needs 1 <= N and 2 N <= T, got (T, N) = ({T}, {N})")
    G2 = _levels(T, 2 * N)
    G = G2[::2]
    if any(a <= b for a, b in zip(G2[:-1], G2[1:])):
        raise ValueError(f"the teacher's grid at 2 N steps does not decrease strictly for (T, N) = ({T}, {N})")
    if G != _levels(T, N):
        raise ValueError(f"the student's grid is not every second level of the teacher's for (T, N) = ({T}, {N}): "
                         "ddim_sample at N steps would walk other timesteps than the ones trained")
    return G, G2


def schedule64(gd):
    """(alpha, sigma, sqrt_recip, sqrt_recipm1) by timestep as float64 host tensors: the diffusion's float32 tables, read exactly"""
    return tuple(getattr(gd, n).detach().double().cpu() for n in
                 ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                  "sqrt_recipm1_alphas_cumprod"))


def plan_row(sched, t: int, t_mid: int, t_next: int) -> List[float]:
    """one float64 row (module text; csrc/distill.hip) for the levels t > t_mid > t_next >= -1"""
    a, s, r, rm1 = sched
    an, sn = (1.0, 0.0) if t_next < 0 else (float(a[t_next]), float(s[t_next]))
    at, st = float(a[t]), float(s[t])
    ratio = sn / st
    den = an - ratio * at
    return [at, st, float(r[t]), float(rm1[t]), float(a[t_mid]), float(s[t_mid]), float(r[t_mid]), float(rm1[t_mid]),
            an, sn, 1.0 / den, -ratio / den, 1.0 / st, float(t_mid), den, float(t_next)]


def distill_plan(gd, N: int) -> torch.Tensor:
    """float64 [T, 16]: row G[i] for i < N as ``plan_row`` says, NaN in every other row (a timestep off the student's grid is
    never read; a wrong index shows)."""
    T = int(gd.num_timesteps)
    G, G2 = distill_grid(T, N)
    sched = schedule64(gd)
    rows = torch.full((T, ROW), math.nan, dtype=torch.float64)
    for i in range(N):
        row = plan_row(sched, G[i], G2[2 * i + 1], G[i + 1])
        if not row[DEN] > 0.0:
            raise ValueError(f"the schedule does not separate levels {G[i]} and {G[i + 1]}: den = {row[DEN]!r}")
        rows[G[i]] = torch.tensor(row, dtype=torch.float64)
    return rows


_SCHEDULE_TABLES = ("betas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                    "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")


def check_arguments(student, teacher, steps) -> int:
    """The refusals of ``GaussianDiffusion.distill_from`` (listed there) -> N.  ``student`` / ``teacher``: diffusions."""
    if isinstance(steps, bool) or not isinstance(steps, int):
        raise ValueError(f"steps must be an int (the student's number of sampling steps), got {steps!r}")
    for what, on in (("self_condition", student.self_condition), ("learned_variance", student.learned_variance),
                     ("lowres_cond", student.lowres_cond), ("dropout > 0", float(getattr(student.model, "dropout", 0.0)) > 0.0),
                     ("offset_noise_strength > 0", float(student.offset_noise_strength) > 0.0)):
        if on:
            raise NotImplementedError(f"distillation of a student with {what} is not built")
    if student.t_sampler != "uniform":
        raise NotImplementedError(f"distillation draws its level uniformly: t_sampler={student.t_sampler!r} is not built")
    if student.sampler == "dpm++":
        raise ValueError("a distilled student is sampled by ddim_sample: sampler='dpm++' cannot be combined with a teacher")
    for what in ("self_condition", "learned_variance", "lowres_cond"):
        if getattr(teacher, what):
            raise NotImplementedError(f"distillation from a teacher with {what} is not built")
    if teacher.objective not in ("pred_noise", "pred_x0", "pred_v"):
        raise ValueError(f"unknown teacher objective {teacher.objective!r}")
    same = (("channels", student.channels, teacher.channels), ("img_size", student.img_size, teacher.img_size),
            ("num_timesteps", student.num_timesteps, teacher.num_timesteps),
            ("num_classes", student.num_classes, teacher.num_classes))
    for what, mine, theirs in same:
        if mine != theirs:
            raise ValueError(f"the teacher's {what} differs from the student's: {theirs!r} and {mine!r}")
    for n in _SCHEDULE_TABLES:
        if not torch.equal(getattr(student, n).detach().cpu(), getattr(teacher, n).detach().cpu()):
            raise ValueError(f"the teacher's schedule table {n} differs from the student's")
    if 2 * steps > student.num_timesteps:
        raise ValueError(f"2 * steps > T: a teacher of {2 * steps} steps does not fit {student.num_timesteps} timesteps")
    distill_grid(student.num_timesteps, steps)
    return steps
