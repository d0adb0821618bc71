"""float64 numpy restatement of the progressive-distillation target (csrc/distill.hip, lgm_hip/distill.py) and its error bound.
No device, no library, no import of the code under test.

With a_s = alpha[s], s_s = sigma[s] (a_-1 = 1, s_-1 = 0), R_s = 1 / a_s given as ``recip[s]`` and Rm1_s = s_s / a_s as
``recipm1[s]``, a teacher of objective ``obj_t`` and the student's ``obj_s`` (0 pred_noise, 1 pred_x0, 2 pred_v):

    pred(z, o, s)   x0 = o (1) | R_s z - Rm1_s o (0) | a_s z - s_s o (2);  clip: x0 = clamp(x0, -1, 1);
                    e  = o when obj_t = 0 and not clip, else (R_s z - x0) / Rm1_s
    step 2          (x1, e1) = pred(z_t, o1, t);    z_t'  = a_t' x1 + s_t' e1
    step 3          (x2, e2) = pred(z_t', o2, t');  z_t'' = a_t'' x2 + s_t'' e2
    step 4          x~ = (z_t'' - r z_t) / den,  r = s_t'' / s_t,  den = a_t'' - r a_t
    step 5          x~ | e~ = (z_t - a_t x~) / s_t | a_t e~ - s_t x~

Every function returns (value, mag): ``mag`` is the same expression with every operand replaced by its magnitude and every
difference by a sum - the M / den of the bound: it carries the 1 / den of step 4 and what step 5 multiplies it by.  A float32
evaluation whose longest path has k roundings is within about k u mag of the exact value (clamp is 1-Lipschitz and only lowers
magnitudes); the tests assert (k + 2) u mag with k from ``ROUNDINGS``, counted along the kernel's own order of operations with one
rounding per table coefficient (float64 rounded once), per product, per sum and per quotient:

    pred: x0 3 (coefficient, product, difference), e 6 (x0's 3 behind R z's 2 -> difference 4, coefficient and quotient 6)
    half step: z_t' = 6 + 2 (coefficient, product) + 1 (sum) = 9
    target: z_t'' 9, x~ = 9 + 2 + 1 = 12, e~ = 12 + 2 (a_t x~) + 1 (difference) + 2 (coefficient 1 / s_t, product) = 17,
            v~ = 17 + 2 + 1 = 20
"""
import numpy as np

U = 2.0 ** -24                        # unit roundoff of float32
ROUNDINGS = {"half": 9, 1: 12, 0: 17, 2: 20}     # the half step's z_t'; the target by student objective


def grids(T, N):
    """(G, G2) as the definition words them: G2 = reversed(torch.linspace(-1, T - 1, 2 N + 1).int()), G = G2[::2] - torch's own
    float32 linspace, whose truncation is what ``ddim_time_pairs`` walks (numpy's differs in the last bit of some levels)"""
    import torch
    G2 = torch.linspace(-1, T - 1, 2 * N + 1).int().tolist()[::-1]
    return G2[::2], G2


def coefficients(alpha, sigma, recip, recipm1, t, t_mid, t_next):
    """the 16 float64 values of the table row at t, in the kernel's order"""
    an, sn = (1.0, 0.0) if t_next < 0 else (float(alpha[t_next]), float(sigma[t_next]))
    r = sn / float(sigma[t])
    den = an - r * float(alpha[t])
    return np.array([alpha[t], sigma[t], recip[t], recipm1[t], alpha[t_mid], sigma[t_mid], recip[t_mid], recipm1[t_mid],
                     an, sn, 1.0 / den, -r / den, 1.0 / float(sigma[t]), float(t_mid), den, float(t_next)], dtype=np.float64)


def pred(z, o, head, obj_t, clip):
    """-> (x0, e, mag x0, mag e, clipped mask) of the teacher's model_predictions with rederive_pred_noise"""
    A, S, R, Rm1 = head
    za, oa = np.abs(z), np.abs(o)
    if obj_t == 1:
        x0, x0m = o.copy(), oa.copy()
    elif obj_t == 0:
        x0, x0m = R * z - Rm1 * o, R * za + Rm1 * oa
    else:
        x0, x0m = A * z - S * o, A * za + S * oa
    hit = np.abs(x0) > 1.0
    if clip:
        x0 = np.clip(x0, -1.0, 1.0)
    if obj_t == 0 and not clip:
        return x0, o.copy(), x0m, oa.copy(), hit
    return x0, (R * z - x0) / Rm1, x0m, (R * za + x0m) / Rm1, hit


def half_step(z_t, o1, row, obj_t, clip):
    """-> (z_t', mag, clipped mask); per-sample ``row`` [B, 16] broadcast over [B, C, H, W]"""
    c = row.reshape(row.shape[0], 16, 1, 1, 1)
    x1, e1, x1m, e1m, hit = pred(z_t, o1, (c[:, 0], c[:, 1], c[:, 2], c[:, 3]), obj_t, clip)
    return c[:, 4] * x1 + c[:, 5] * e1, c[:, 4] * x1m + c[:, 5] * e1m, hit


def target(z_t, z_mid, o2, row, obj_t, obj_s, clip):
    """-> (target in the student's objective, mag, x~, clipped mask)"""
    c = row.reshape(row.shape[0], 16, 1, 1, 1)
    x2, e2, x2m, e2m, hit = pred(z_mid, o2, (c[:, 4], c[:, 5], c[:, 6], c[:, 7]), obj_t, clip)
    zn, znm = c[:, 8] * x2 + c[:, 9] * e2, c[:, 8] * x2m + c[:, 9] * e2m
    xs, xsm = c[:, 10] * zn + c[:, 11] * z_t, np.abs(c[:, 10]) * znm + np.abs(c[:, 11]) * np.abs(z_t)
    es, esm = (z_t - c[:, 0] * xs) * c[:, 12], (np.abs(z_t) + c[:, 0] * xsm) * c[:, 12]
    vs, vsm = c[:, 0] * es - c[:, 1] * xs, c[:, 0] * esm + c[:, 1] * xsm
    val, mag = {1: (xs, xsm), 0: (es, esm), 2: (vs, vsm)}[obj_s]
    return val, mag, xs, hit


def two_teacher_steps(z_t, teacher, alpha, sigma, recip, recipm1, t, t_mid, t_next, obj_t, clip):
    """steps 2 - 4 with ``teacher(z, s) -> o`` called twice, for ONE level triple shared by the batch -> (x~, z_t'')"""
    row = coefficients(alpha, sigma, recip, recipm1, t, t_mid, t_next)[None].repeat(z_t.shape[0], 0)
    z_mid, _, _ = half_step(z_t, teacher(z_t, t), row, obj_t, clip)
    c = row.reshape(row.shape[0], 16, 1, 1, 1)
    x2, e2, _, _, _ = pred(z_mid, teacher(z_mid, t_mid), (c[:, 4], c[:, 5], c[:, 6], c[:, 7]), obj_t, clip)
    zn = c[:, 8] * x2 + c[:, 9] * e2
    return c[:, 10] * zn + c[:, 11] * z_t, zn


def student_ddim_step(z_t, x0, alpha, sigma, t, t_next):
    """one DDIM step (eta = 0) of a student whose x0 prediction at (z_t, t) is ``x0``"""
    if t_next < 0:
        return x0
    eps = (z_t - alpha[t] * x0) / sigma[t]
    return alpha[t_next] * x0 + sigma[t_next] * eps
