"""float64 restatement of the low-resolution conditioning slice (csrc/lowres.hip, ``lgm_lowres_cond``) and its error bound.

    l   = mean of img over r x r blocks                       (or the given low-resolution image)
    n   = 2 l - 1                                             when ``normalize``
    u   = bilinear upsample of n by r, align_corners=False:   source coordinate (dst + 0.5) / r - 0.5 clamped at 0, the
          upper tap clamped at the last row / column
    c   = sqrt_ac[s] u + sqrt_1mac[s] eps                     (``eps`` None: c = u)

``M`` is the sum of the magnitudes of the terms, as the other kernel tests define it: every product and sum above with its
operands replaced by their magnitudes (|2 l - 1| by 2 mean|x| + 1).  A float32 evaluation whose longest path has k roundings
is within about k u M of the exact value; the tests assert (k + 2) u M with k from ``roundings``.  No GPU, no library."""
import math

import torch

U = 2.0 ** -24                        # unit roundoff of float32


def area_mean(x, r):
    """float64 mean over r x r blocks of [B, C, H, W]"""
    B, C, H, W = x.shape
    return x.double().reshape(B, C, H // r, r, W // r, r).mean((3, 5))


def area_mean_f32(x, r):
    """the float32 average the kernel's training source forms: every row of r by the halving tree v[i] += v[i + n/2], the r
    row sums by the same tree, times 1 / r^2"""
    B, C, H, W = x.shape
    v = x.float().reshape(B, C, H // r, r, W // r, r)
    n = r
    while n > 1:                                               # along dx
        v = v[..., :n // 2] + v[..., n // 2:n]
        n //= 2
    v = v[..., 0]                                              # [B, C, h, r(dy), w]
    n = r
    while n > 1:                                               # along dy
        v = v[:, :, :, :n // 2] + v[:, :, :, n // 2:n]
        n //= 2
    return v[:, :, :, 0] * (1.0 / (r * r))


def taps(n_low, r):
    """(i0, i1, w0, w1) of the n_low * r outputs along one axis, float64"""
    src = ((torch.arange(n_low * r, dtype=torch.float64) + 0.5) / r - 0.5).clamp_min(0.0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp_max(n_low - 1)
    w1 = src - i0
    return i0, i1, 1.0 - w1, w1


def upsample(l, r):
    """bilinear, align_corners=False, of float64 [B, C, h, w] by the integer factor r"""
    h, w = l.shape[-2:]
    y0, y1, wy0, wy1 = taps(h, r)
    x0, x1, wx0, wx1 = taps(w, r)
    top = l[:, :, y0][..., x0] * wx0 + l[:, :, y0][..., x1] * wx1
    bot = l[:, :, y1][..., x0] * wx0 + l[:, :, y1][..., x1] * wx1
    return top * wy0[:, None] + bot * wy1[:, None]


def cond_slice(r, img=None, low=None, normalize=True, sqrt_ac=None, sqrt_1mac=None, s=None, eps=None):
    """-> (c, M), float64 [B, C, H, W] each.  Exactly one of ``img`` (data at full size) / ``low``; tables and ``s`` are read
    with ``eps`` only, ``s`` clamped into the table."""
    assert (img is None) != (low is None)
    l = area_mean(img, r) if img is not None else low.double()
    la = area_mean(img.abs(), r) if img is not None else low.double().abs()
    n, na = (2 * l - 1, 2 * la + 1) if normalize else (l, la)
    u, ua = upsample(n, r), upsample(na, r)
    if eps is None:
        return u, ua
    si = s.long().clamp(0, sqrt_ac.shape[0] - 1)
    a = sqrt_ac.double()[si].view(-1, 1, 1, 1)
    b = sqrt_1mac.double()[si].view(-1, 1, 1, 1)
    return a * u + b * eps.double(), a.abs() * ua + b.abs() * eps.double().abs()


def roundings(r, from_img, normalize, augment):
    """roundings on the longest path of the kernel's expression, in its order: the two halving trees of the average (log2 r
    levels each; the scale by 1 / r^2 is exact), the normalisation's subtraction (2 l is exact), the bilinear taps (tap
    product, row sum, row product, column sum; the weights are exact multiples of 1 / (2 r)), the augmentation (product, sum)"""
    return (2 * int(math.log2(r)) if from_img else 0) + (1 if normalize else 0) + 4 + (2 if augment else 0)
