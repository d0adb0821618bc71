"""Elucidated diffusion (Karras et al. 2022, "Elucidating the Design Space of Diffusion-Based Generative Models"; an extension
of the reference) - the host side: the preconditioning coefficients, the rho-schedule, the churn and the float64 rows the
sampling kernels of csrc/edm.hip read.  Pure Python float64: no device, no library, no torch.

With s_d = ``sigma_data`` (Table 1, "Ours"):

    c_in(s) = 1 / sqrt(s^2 + s_d^2)     c_skip(s) = s_d^2 / (s^2 + s_d^2)     c_out(s) = s s_d / sqrt(s^2 + s_d^2)
    c_noise(s) = ln(s) / 4              lambda(s) = (s^2 + s_d^2) / (s s_d)^2 = 1 / c_out(s)^2
    D(x, s) = c_skip x + c_out F(c_in x, c_noise)

Sampling (Algorithm 2) on N steps:

    s_i = (s_max^(1/rho) + i / (N - 1) (s_min^(1/rho) - s_max^(1/rho)))^rho   for i < N,     s_N = 0
    gamma_i = min(S_churn / N, sqrt(2) - 1) where S_tmin <= s_i <= S_tmax, else 0
    s^ = s_i (1 + gamma_i)      x^ = x + sqrt(s^^2 - s_i^2) S_noise eps
    d  = (x^ - D(x^, s^)) / s^          x' = x^ + (s_{i+1} - s^) d
    d' = (x' - D(x', s_{i+1})) / s_{i+1}    x_{i+1} = x^ + (s_{i+1} - s^) (d + d') / 2       where s_{i+1} > 0

A row of ``edm_plan`` is everything one step's launches read, each entry formed in float64 and rounded once by the caller:

    0..3    s_i   s^   coef = sqrt(s^^2 - s_i^2) S_noise   s_{i+1}
    4..7    c_in  c_noise  c_skip  c_out      at s^
    8..11   the same at s_{i+1}  (zeros when s_{i+1} = 0)
    12      dt = s_{i+1} - s^
    13      gamma_i
    14..15  0"""
from __future__ import annotations

import math
from typing import List, Optional

ROW = 16           # floats per row (csrc/edm.hip)
(S_I, S_HAT, COEF, S_NEXT, CIN, CNOISE, CSKIP, COUT, CIN_N, CNOISE_N, CSKIP_N, COUT_N, DT, GAMMA, _R14, _R15) = range(ROW)
GAMMA_MAX = math.sqrt(2.0) - 1.0


def check_arguments(num_sample_steps, sigma_min, sigma_max, sigma_data, rho, P_std, S_churn):
    """ValueError by name for every argument outside its range"""
    if not float(sigma_min) > 0.0:
        raise ValueError(f"sigma_min must be positive, got {sigma_min!r}")
    if not float(sigma_max) > float(sigma_min):
        raise ValueError(f"sigma_max must exceed sigma_min = {sigma_min!r}, got {sigma_max!r}")
    if not float(sigma_data) > 0.0:
        raise ValueError(f"sigma_data must be positive, got {sigma_data!r}")
    if not float(rho) > 0.0:
        raise ValueError(f"rho must be positive, got {rho!r}")
    check_steps(num_sample_steps, "num_sample_steps")
    if not float(S_churn) >= 0.0:
        raise ValueError(f"S_churn must not be negative, got {S_churn!r}")
    if not float(P_std) > 0.0:
        raise ValueError(f"P_std must be positive, got {P_std!r}")


def check_steps(steps, name: str = "steps") -> int:
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 2:
        raise ValueError(f"{name} must be an integer of at least 2, got {steps!r}")
    return int(steps)


def coefficients(sigma: float, sigma_data: float):
    """(c_in, c_noise, c_skip, c_out) at ``sigma`` > 0"""
    s2 = sigma * sigma + sigma_data * sigma_data
    r = math.sqrt(s2)
    return 1.0 / r, 0.25 * math.log(sigma), sigma_data * sigma_data / s2, sigma * sigma_data / r


def loss_weight(sigma: float, sigma_data: float) -> float:
    """lambda(sigma) = 1 / c_out^2"""
    return (sigma * sigma + sigma_data * sigma_data) / (sigma * sigma_data) ** 2


def sigma_grid(N: int, sigma_min: float, sigma_max: float, rho: float) -> List[float]:
    """the N + 1 levels: s_0 = sigma_max, s_{N-1} = sigma_min (both exactly), s_N = 0"""
    N = check_steps(N)
    a, b = sigma_max ** (1.0 / rho), sigma_min ** (1.0 / rho)
    grid = [(a + i / (N - 1) * (b - a)) ** rho for i in range(N)]
    grid[0], grid[-1] = float(sigma_max), float(sigma_min)       # the ends as given, not as the power round trip leaves them
    return grid + [0.0]


def gammas(grid: List[float], S_churn: float, S_tmin: float, S_tmax: float) -> List[float]:
    """gamma_i per step of ``grid`` (len(grid) - 1 entries)"""
    N = len(grid) - 1
    g = min(float(S_churn) / N, GAMMA_MAX)
    return [g if S_tmin <= s <= S_tmax else 0.0 for s in grid[:-1]]


def edm_plan(N: int, *, sigma_min: float, sigma_max: float, sigma_data: float, rho: float, S_churn: float = 0.0,
             S_tmin: float = 0.05, S_tmax: float = 50.0, S_noise: float = 1.003, grid: Optional[List[float]] = None):
    """-> N rows of ``ROW`` float64 values, one per step of the chain"""
    grid = sigma_grid(N, sigma_min, sigma_max, rho) if grid is None else list(grid)
    rows = []
    for i, gamma in enumerate(gammas(grid, S_churn, S_tmin, S_tmax)):
        s, nxt = grid[i], grid[i + 1]
        hat = s * (1.0 + gamma)
        row = [0.0] * ROW
        row[S_I], row[S_HAT], row[S_NEXT], row[GAMMA] = s, hat, nxt, gamma
        row[COEF] = math.sqrt(max(hat * hat - s * s, 0.0)) * float(S_noise) if gamma > 0.0 else 0.0
        row[CIN:COUT + 1] = coefficients(hat, sigma_data)
        if nxt > 0.0:
            row[CIN_N:COUT_N + 1] = coefficients(nxt, sigma_data)
        row[DT] = nxt - hat
        rows.append(row)
    return rows
