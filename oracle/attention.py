"""Float64 references, per-element error scales and float32 CPU evaluations of the attention cores of the DDPM UNet -
LinearAttention (ddpm.py:217-239) and full softmax attention with memory rows (ddpm.py:255-271) - forward and backward, for
the ledger of the attention kernels (tests/test_hip_attention_ledger.py).  CPU code, no GPU.

Layout.  LinearAttention: q, k, v [B, heads, 32, n], mem [2, heads, 32, M], gout [B, heads, 32, n]; the keys run in the
kernels' order, the n pixels and then the M memory columns.  Full attention: q, k, v [B, heads, n, 32], mem [2, heads, M, 32],
gout [B, heads, n, 32]; the M memory rows come first.  Every function takes its operands in a dict ``t`` and evaluates in the
dtype of those tensors, so the same code gives the float64 reference and a float32 evaluation in torch's own order.

The scale S of an output follows the rule of oracle/bounds.py - the same formula with every term replaced by its absolute
value, differences become sums - so that a float32 evaluation in ANY order has an error of a few 2^-24 * S per element.
Through the non-linear steps the rule is applied to the first-order propagation (R(.) is a relative scale: S = |value| R):

  * e = exp(t), t <= 0.  The kernels use the hardware exponential, exp2(t * log2(e)): the rounded constant and the rounded
    product each change the argument by 2^-24 |t| log2(e) (a relative error 2^-24 |t| of e), the exp2 itself is good to an
    ulp = 2 * 2^-24 (the derivation is in oracle/norm.py): R(e) = E(t) = 2 |t| + 2.  Derived, not measured.  Where the
    argument itself carries an absolute scale S_t (a logit that is a float32 dot product), R(e) = E(t) + S_t.
    A running maximum splits t = (k - m_1) + (m_1 - m_2) + ... into terms of one sign whose absolute values add up to |t|:
    the argument part of E is the same, and each further factor adds one exp2 (2 units) - but the SAME factor multiplies the
    accumulator and the partial sum, so it cancels in every normalised output and stays only in ksum.
  * a softmax weight p_j = e_j / sum e: the sum has the scale sum_j e_j R(e_j) + sum_j e_j (the plain summation term), so
    R(p_j) = R(e_j) + Rbar + 2 with Rbar = sum_j p_j R(e_j) (one unit for the sum, one for the division).
    A maximum is exact and cancels in p: it has no term.
  * LinearAttention forward: t = k - kmax.  S_ksum = ksum (Rbar + 1).  ks = softmax_n(k): S_ks = ks R(ks).
    ctx[d][e] = sum_j ks[d][j] v[e][j]: S_ctx = sum_j S_ks |v|.  qs = softmax_d(q), S_qs alike.
    out = scale sum_d ctx qs: S_out = scale sum_d (S_ctx qs + |ctx| S_qs): the scale of ctx is carried through the product.
  * LinearAttention backward, from the SAVED ctx / kmax / ksum (so ks inherits the scale of ksum, which R(ks) already holds):
    gctx = scale sum_i qs gout: S = scale sum_i S_qs |gout|.  T1 = sum_e ctx gout: S = sum_e S_ctx |gout|; g1 = scale T1;
    dot = sum_d qs g1: S = sum_d (S_qs |g1| + qs S_g1); gq = qs (g1 - dot): S = S_qs (|g1| + |dot|) + qs (S_g1 + S_dot).
    gv = sum_d ks gctx: S = sum_d (S_ks |gctx| + ks S_gctx).  T2 = sum_e gctx v: S = sum_e S_gctx |v|;
    r = sum_e gctx ctx: S = sum_e (S_gctx |ctx| + |gctx| S_ctx); gk = ks (T2 - r): S = S_ks (|T2| + |r|) + ks (S_T2 + S_r).
    The memory columns' gradient is the sum over the images of gk / gv at the memory columns (+ |previous value| at beta = 1).
  * Full attention forward: s = scale q . k with S_s = scale sum_d |q||k|; t = s - max s; R(e) = E(t) + S_s.
    out = sum_j p_j v_j: S = sum_j S_p |v|.  lse = m + ln(den): the maximum cancels (lse = ln sum exp s whatever m is), the sum
    carries Rbar + 1 relative, i.e. absolute in ln, and the hardware logarithm log2(den) ln 2 two roundings of its value:
    S_lse = |m| + 3 |ln den| + Rbar + 1.
  * Full attention backward, from the SAVED out and lse: p = exp(s - lse): R(p) = E(s - lse) + S_s + S_lse (+ 1 for p itself).
    delta = sum_d gout out: S = sum_d |gout| S_out.  dp = sum_d gout v: S = sum |gout||v|.
    ds = p (dp - delta): S = S_p (|dp| + |delta|) + p (S_dp + S_delta).  gq = scale sum_j ds k, gk = scale sum_i ds q,
    gv = sum_i p gout: the scales S_ds and S_p carried through the products.

Inputs.  Every exponent argument of every live weight stays within [-60, 0] (asserted where the operands are built: a
condition on the inputs, so that no weight flushes to zero in float32).  Families: see ``la_inputs`` / ``fa_inputs``.

The tolerance constants are measured on the REFERENCE, never on the kernels: tests/test_cpu_attention_bounds.py evaluates
every ledger row in float32 on the CPU - in torch's own order, and "online": key tiles of 64 and of 128 with a running maximum,
an exp(m_old - m_new) rescale and strictly sequential accumulation (written from the definition of online softmax) - scores
them against float64 and asserts the worst score against the constants below.  The kernels get 4 times that (another
summation order), the margin of oracle/bounds.py."""
import numpy as np
import torch

from oracle.bounds import UNIT, forward_error_units, rel  # noqa: F401  (re-exported for the tests)
from oracle.norm import scores, to, worst  # noqa: F401

DH = 32
SCALE = DH ** -0.5
LA_TILE = 128            # rows per tile of linattn_ctx_mfma
FA_TILE = 64             # keys per tile of attn_tiled_fwd_kernel
T_MIN = -60.0

# Worst forward_error_units of a float32 CPU evaluation (torch's order and both online orders) over every ledger row and
# output, measured by tests/test_cpu_attention_bounds.py and rounded up:
#   * LinearAttention (core and fused tails): 1.75, ksum of the n = 128 "memmax" row in torch's order (the online orders: 1.04,
#     ksum of the three-tile "ascending" row; the gradients 0.5 ... 1.0; the fused tails 0.01 ... 0.96).
#   * full attention: 2.46, lse of the n + M = 192 "memmax" row in all three orders (out and the gradients: under 1).
# The weakest mutation on a row named for it scores 284.6 (LinearAttention: memory columns left out of ksum at the fused
# forward tail of the n = 129 "late" row) and 310.9 (full attention: a memory row read with the wrong stride at n = 65).
C_LINATTN_REF_WORST = 2.0
C_ATTN_REF_WORST = 3.0


def tolerance(family="attn") -> float:
    """units of 2^-24 * S: four times the worst float32 reference of the family: "attn" = full attention, every other kind
    of row (the LinearAttention core and its fused tails) = "linattn"."""
    return 4.0 * (C_ATTN_REF_WORST if family == "attn" else C_LINATTN_REF_WORST)


# the mutations a subtly wrong kernel would leave (applied to a float32 evaluation of a row's own inputs)
M_ACC = "accumulator not rescaled when the maximum moves in the last tile"
M_WSUM = "partial sum (wsum) not rescaled when the maximum moves in the last tile"
M_KSUM_MEM = "memory columns left out of ksum"
M_DROP = "last pixel of a ragged tile dropped"
M_STRIDE = "one memory column read with the wrong stride"
M_SCALE2 = "scale applied twice to gq"
M_LSE = "lse without its maximum"
M_DELTA = "delta_i taken from the unnormalised output"
M_HEAD = "head index bh / heads in place of bh % heads"
M_RVEC = "rvec left out of gk"


def E(t):
    """relative scale of the hardware exponential of the argument t"""
    return 2 * t.abs() + 2


def _ramp(n, top, dtype=torch.float32):
    return torch.linspace(0.0, top, n, dtype=dtype) if n > 1 else torch.full((1,), top, dtype=dtype)


# =============================================================================================================================
# memory columns / rows with the mutations of their addressing
# =============================================================================================================================
def _mem(t, mut, la):
    """(mk, mv) [B, heads, ...] of the batch.  M_HEAD: image b, head h reads the head (b * heads + h) // heads = b.
    M_STRIDE: memory column 1 is read from the flat [32][M] (LinearAttention) / [M][32] (full attention) block with the other
    layout's stride."""
    mem, B = t["mem"], t["q"].shape[0]
    heads = mem.shape[1]
    M = mem.shape[3] if la else mem.shape[2]
    if mut == M_STRIDE and M >= 2:
        mem = mem.clone()
        flat = t["mem"].reshape(2, heads, DH * M)
        d = torch.arange(DH)
        if la:                                     # [d][j] lives at d * M + j; read at j * 32 + d
            mem[:, :, :, 1] = flat[:, :, 1 * DH + d]
        else:                                      # [j][d] lives at j * 32 + d; read at d * M + j
            mem[:, :, 1, :] = flat[:, :, d * M + 1]
    if mut == M_HEAD:
        idx = torch.tensor([[(b * heads + h) // heads for h in range(heads)] for b in range(B)]) % heads
        return mem[0][idx], mem[1][idx]
    return tuple(m.unsqueeze(0).expand(B, -1, -1, -1) for m in mem)


# =============================================================================================================================
# LinearAttention
# =============================================================================================================================
def la_inputs(geom, family="plain", seed=0):
    """geom = (B, heads, H, W, M).  Families (k in the kernels' row order: pixels, then memory columns):
    "plain": 1.5 N(0, 1), what the per-op tests use; "ascending": k = N(0, 0.5) + a ramp of 12 across the n + M rows (the
    running maximum moves at every tile); "late": the last pixel's k is 12 higher; "memmax": memory column 0 sits at 16, about
    12 above every pixel key; "spike": the last pixel's k and one channel of q sit 20 above the rest (every other weight is about e^-20, below
    2^-24 of the sums)."""
    B, heads, H, W, M = geom
    n = H * W
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q, k, v = 1.5 * r(B, heads, DH, n), 1.5 * r(B, heads, DH, n), 1.5 * r(B, heads, DH, n)
    mem = r(2, heads, DH, M)
    if family == "ascending":
        ramp = _ramp(n + M, 12.0)
        k = 0.5 * r(B, heads, DH, n) + ramp[:n]
        mem[0] = 0.5 * mem[0] + ramp[n:]
    elif family == "late":
        k = r(B, heads, DH, n)
        k[..., n - 1] += 12.0
    elif family == "memmax":
        k = r(B, heads, DH, n)
        mem[0, :, :, 0] = 16.0 + 0.5 * mem[0, :, :, 0]
    elif family == "spike":
        k[..., n - 1] += 20.0
        q[:, :, 5, :] += 20.0
    else:
        assert family == "plain", family
    t = {"q": q, "k": k, "v": v, "mem": mem, "gout": r(B, heads, DH, n), "gm0": r(2, heads, DH, M)}
    mk, _ = _mem(t, None, True)
    kk = torch.cat((k, mk), -1).double()
    assert float((kk - kk.max(-1, keepdim=True).values).min()) >= T_MIN, "a key weight would flush to zero in float32"
    assert float((q.double() - q.double().max(-2, keepdim=True).values).min()) >= T_MIN
    return t


def _la_keys(t, mut=None):
    mk, mv = _mem(t, mut, True)
    return torch.cat((t["k"], mk), -1), torch.cat((t["v"], mv), -1)


def la_out(t, ctx):
    qs = t["q"].softmax(-2)
    return torch.einsum("bhde,bhdi->bhei", ctx, qs) * SCALE


def la_forward(t, mut=None):
    """-> {kmax, ksum [B, heads, 32]; ctx [B, heads, 32, 32]; out [B, heads, 32, n]}"""
    kk, vv = _la_keys(t, mut)
    n = t["k"].shape[-1]
    if mut == M_DROP:
        kk, vv = (torch.cat((a[..., :n - 1], a[..., n:]), -1) for a in (kk, vv))
        n -= 1
    kmax = kk.max(-1).values
    e = torch.exp(kk - kmax[..., None])
    ksum = (e[..., :n] if mut == M_KSUM_MEM else e).sum(-1)
    ctx = torch.einsum("bhdj,bhej->bhde", e, vv) / ksum[..., None]
    return {"kmax": kmax, "ksum": ksum, "ctx": ctx, "out": la_out(t, ctx)}


def _seq_add(base, e, v=None):
    """base + sum_j e[..., j] (v is None) or base[..., c] + sum_j e[..., j] v[..., c, j], along the last axis in float32 with
    one addition per term in index order (image by image: the products of a whole batch need not exist at once)"""
    out = []
    for i in range(base.shape[0]):
        x = e[i] if v is None else e[i][:, :, None, :] * v[i][:, None, :, :]
        out.append(np.cumsum(np.concatenate([base[i][..., None], x], -1), axis=-1, dtype=np.float32)[..., -1])
    return np.stack(out)


def la_forward_online(t, tile, mut=None):
    """float32, from the definition of online softmax: per column d a running maximum over tiles of ``tile`` rows, the sums
    so far rescaled by exp(m_old - m_new), every sum one addition per row."""
    f = np.float32
    kk, vv = (a.numpy().astype(f) for a in _la_keys(t))
    total = kk.shape[-1]
    m = np.full(kk.shape[:-1], -np.inf, f)
    den = np.zeros(kk.shape[:-1], f)
    acc = np.zeros(kk.shape[:-1] + (DH,), f)
    for j0 in range(0, total, tile):
        kt, vt = kk[..., j0:j0 + tile], vv[..., j0:j0 + tile]
        mn = np.maximum(m, kt.max(-1))
        corr = np.exp(m - mn).astype(f)
        last = j0 > 0 and j0 + tile >= total
        e = np.exp(kt - mn[..., None]).astype(f)
        den = _seq_add(den if (mut == M_WSUM and last) else den * corr, e)
        acc = _seq_add(acc if (mut == M_ACC and last) else acc * corr[..., None], e, vt)
        m = mn
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(f)))
    ctx = c(acc / den[..., None])
    return {"kmax": c(m), "ksum": c(den), "ctx": ctx, "out": la_out(t, ctx)}


def la_backward(t, sv, beta=0.0, mut=None):
    """From the saved ctx / kmax / ksum ``sv`` -> {gqkv [B, 3, heads, 32, n]; gmem [2, heads, 32, M]}."""
    kk, vv = _la_keys(t)
    n, gout, ctx = t["k"].shape[-1], t["gout"], sv["ctx"]
    ks = torch.exp(kk - sv["kmax"][..., None]) / sv["ksum"][..., None]
    qs = t["q"].softmax(-2)
    gctx = torch.einsum("bhdi,bhei->bhde", qs, gout) * SCALE
    g1 = torch.einsum("bhde,bhei->bhdi", ctx, gout) * SCALE
    gq = qs * (g1 - (qs * g1).sum(-2, keepdim=True))
    if mut == M_SCALE2:
        gq = gq * SCALE
    gv = torch.einsum("bhdj,bhde->bhej", ks, gctx)
    T2 = torch.einsum("bhde,bhej->bhdj", gctx, vv)
    r = (gctx * ctx).sum(-1)
    gk = ks * (T2 if mut == M_RVEC else T2 - r[..., None])
    gmem = torch.stack((gk[..., n:].sum(0), gv[..., n:].sum(0)))
    return {"gqkv": torch.stack((gq, gk[..., :n], gv[..., :n]), 1), "gmem": gmem + beta * t["gm0"] if beta else gmem}


def _softmax_scale(e_over_sum, R):
    """S of p = e / sum e along the LAST axis from the relative scale R of e: p (R + Rbar + 2); also Rbar"""
    Rbar = (e_over_sum * R).sum(-1, keepdim=True)
    return e_over_sum * (R + Rbar + 2), Rbar


def la_reference(t, beta=0.0):
    """(ref, S): the float64 results of la_forward + la_backward and their scales (module docstring)"""
    d = to(t, torch.float64)
    ref = la_forward(d)
    ref.update(la_backward(d, ref, beta))
    kk, vv = _la_keys(d)
    n, gout, ctx = d["k"].shape[-1], d["gout"].abs(), ref["ctx"]
    tk = kk - ref["kmax"][..., None]
    ks = torch.exp(tk) / ref["ksum"][..., None]
    S_ks, Rbar = _softmax_scale(ks, E(tk))
    S = {"ksum": ref["ksum"] * (Rbar[..., 0] + 1)}
    S_ctx = S["ctx"] = torch.einsum("bhdj,bhej->bhde", S_ks, vv.abs())
    qs = d["q"].softmax(-2)
    tq = d["q"] - d["q"].max(-2, keepdim=True).values
    S_qs = _softmax_scale(qs.transpose(-1, -2), E(tq).transpose(-1, -2))[0].transpose(-1, -2)
    S["out"] = SCALE * (torch.einsum("bhde,bhdi->bhei", S_ctx, qs) + torch.einsum("bhde,bhdi->bhei", ctx.abs(), S_qs))
    # backward
    gctx = torch.einsum("bhdi,bhei->bhde", qs, d["gout"]) * SCALE
    S_gctx = SCALE * torch.einsum("bhdi,bhei->bhde", S_qs, gout)
    g1 = torch.einsum("bhde,bhei->bhdi", ctx, d["gout"]) * SCALE
    S_g1 = SCALE * torch.einsum("bhde,bhei->bhdi", S_ctx, gout)
    dot = (qs * g1).sum(-2, keepdim=True)
    S_dot = (S_qs * g1.abs() + qs * S_g1).sum(-2, keepdim=True)
    S_gq = S_qs * (g1.abs() + dot.abs()) + qs * (S_g1 + S_dot)
    S_gv = torch.einsum("bhdj,bhde->bhej", S_ks, gctx.abs()) + torch.einsum("bhdj,bhde->bhej", ks, S_gctx)
    T2 = torch.einsum("bhde,bhej->bhdj", gctx, vv)
    S_T2 = torch.einsum("bhde,bhej->bhdj", S_gctx, vv.abs())
    r = (gctx * ctx).sum(-1)[..., None]
    S_r = (S_gctx * ctx.abs() + gctx.abs() * S_ctx).sum(-1)[..., None]
    S_gk = S_ks * (T2.abs() + r.abs()) + ks * (S_T2 + S_r)
    S["gqkv"] = torch.stack((S_gq, S_gk[..., :n], S_gv[..., :n]), 1)
    S["gmem"] = torch.stack((S_gk[..., n:].sum(0), S_gv[..., n:].sum(0))) + (beta * d["gm0"].abs() if beta else 0.0)
    return ref, S


def la_autograd64(t):
    """float64 autograd of the textbook definition (ddpm.py:227-237) -> out, gqkv, gmem"""
    d = to(t, torch.float64)
    q, k, v, mem = (d[x].clone().requires_grad_(True) for x in ("q", "k", "v", "mem"))
    B = q.shape[0]
    mk, mv = (m.unsqueeze(0).expand(B, -1, -1, -1) for m in mem)
    kk, vv = torch.cat((mk, k), -1), torch.cat((mv, v), -1)
    ctx = torch.einsum("bhdn,bhen->bhde", kk.softmax(-1), vv)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q.softmax(-2) * SCALE)
    out.backward(d["gout"])
    return {"ctx": ctx.detach(), "out": out.detach(), "gqkv": torch.stack((q.grad, k.grad, v.grad), 1), "gmem": mem.grad}


# =============================================================================================================================
# full attention
# =============================================================================================================================
def fa_inputs(geom, family="plain", seed=0):
    """geom = (B, heads, H, W, M).  q = N(0, 1) + a u with a common unit direction u and a = 6, so that a key b u / (a scale)
    adds b to every query's logit.  Families: "plain": N(0, 1) throughout (a = 0); "ascending": a ramp of 12 across the
    M + n keys in the kernels' order; "late": the last key is 12 higher; "memmax": memory row 0 is 12 higher; "spike": the
    last pixel key is 20 higher; "peaked": plain with q scaled so that the widest row of logits spans exactly 50."""
    B, heads, H, W, M = geom
    n = H * W
    g = torch.Generator().manual_seed(2000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q, k, v = r(B, heads, n, DH), r(B, heads, n, DH), r(B, heads, n, DH)
    mem = r(2, heads, M, DH)
    a = 6.0
    u = torch.nn.functional.normalize(r(DH), dim=0)
    lift = lambda b: (b / (a * SCALE)) * u           # added to a key: + b on every logit
    if family in ("ascending", "late", "memmax", "spike"):
        q = q + a * u
    if family == "ascending":
        ramp = _ramp(M + n, 12.0)
        k = 0.5 * k + ramp[M:, None] * lift(1.0)
        mem[0] = 0.5 * mem[0] + ramp[:M, None] * lift(1.0)
    elif family == "late":
        k[:, :, n - 1] += lift(12.0)
    elif family == "memmax":
        mem[0, :, 0] += lift(12.0)
    elif family == "spike":
        k[:, :, n - 1] += lift(20.0)
    elif family == "peaked":
        s = _fa_logits({"q": q.double(), "k": k.double(), "v": v.double(), "mem": mem.double()})[0]
        q = q * (50.0 / float((s.max(-1).values - s.min(-1).values).max())) * 0.999
    else:
        assert family == "plain", family
    t = {"q": q, "k": k, "v": v, "mem": mem, "gout": r(B, heads, n, DH), "gm0": r(2, heads, M, DH)}
    s = _fa_logits(to(t, torch.float64))[0]
    assert float((s - s.max(-1, keepdim=True).values).min()) >= T_MIN, "a softmax weight would flush to zero in float32"
    return t


def _fa_logits(t, mut=None):
    mk, mv = _mem(t, mut, False)
    kk, vv = torch.cat((mk, t["k"]), -2), torch.cat((mv, t["v"]), -2)
    if mut == M_DROP:
        kk, vv = kk[..., :-1, :], vv[..., :-1, :]
    return torch.einsum("bhid,bhjd->bhij", t["q"] * SCALE, kk), kk, vv


def fa_forward(t, mut=None):
    """-> {out [B, heads, n, 32]; lse [B, heads, n]}"""
    s, kk, vv = _fa_logits(t, mut)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    lse = torch.log(den) if mut == M_LSE else m + torch.log(den)
    return {"out": torch.einsum("bhij,bhjd->bhid", e, vv) / den, "lse": lse[..., 0]}


def fa_forward_online(t, tile, mut=None):
    """float32, from the definition of online softmax: per query a running maximum over tiles of ``tile`` keys, numerator and
    denominator rescaled by exp(m_old - m_new), every sum one addition per key."""
    f = np.float32
    s, kk, vv = _fa_logits(t)
    s, vv = s.numpy().astype(f), vv.numpy().astype(f)
    nk = s.shape[-1]
    m = np.full(s.shape[:-1], -np.inf, f)
    den = np.zeros(s.shape[:-1], f)
    acc = np.zeros(s.shape[:-1] + (DH,), f)
    for j0 in range(0, nk, tile):
        st, vt = s[..., j0:j0 + tile], vv[:, :, j0:j0 + tile]
        mn = np.maximum(m, st.max(-1))
        corr = np.exp(m - mn).astype(f)
        last = j0 > 0 and j0 + tile >= nk
        e = np.exp(st - mn[..., None]).astype(f)
        den = _seq_add(den if (mut == M_WSUM and last) else den * corr, e)
        acc = _seq_add(acc if (mut == M_ACC and last) else acc * corr[..., None], e, vt.transpose(0, 1, 3, 2))
        m = mn
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(f)))
    return {"out": c(acc / den[..., None]), "lse": c(m + np.log(den).astype(f))}


def fa_backward(t, sv, beta=0.0, mut=None):
    """From the saved out / lse ``sv`` -> {gqkv [B, 3, heads, n, 32]; gmem [2, heads, M, 32]}."""
    s, kk, vv = _fa_logits(t)
    M, gout = t["mem"].shape[2], t["gout"]
    p = torch.exp(s - sv["lse"][..., None])
    out = sv["out"]
    if mut == M_DELTA:
        out = out * torch.exp(sv["lse"] - s.max(-1).values)[..., None]
    delta = (gout * out).sum(-1, keepdim=True)
    ds = p * (torch.einsum("bhid,bhjd->bhij", gout, vv) - delta)
    gq = torch.einsum("bhij,bhjd->bhid", ds, kk) * SCALE
    if mut == M_SCALE2:
        gq = gq * SCALE
    gk = torch.einsum("bhij,bhid->bhjd", ds, t["q"] * SCALE)
    gv = torch.einsum("bhij,bhid->bhjd", p, gout)
    gmem = torch.stack((gk[:, :, :M].sum(0), gv[:, :, :M].sum(0)))
    return {"gqkv": torch.stack((gq, gk[:, :, M:], gv[:, :, M:]), 1), "gmem": gmem + beta * t["gm0"] if beta else gmem}


def fa_reference(t, beta=0.0):
    """(ref, S): the float64 results of fa_forward + fa_backward and their scales (module docstring)"""
    d = to(t, torch.float64)
    ref = fa_forward(d)
    ref.update(fa_backward(d, ref, beta))
    s, kk, vv = _fa_logits(d)
    M, gout = d["mem"].shape[2], d["gout"]
    S_s = torch.einsum("bhid,bhjd->bhij", d["q"].abs() * SCALE, kk.abs())
    m = s.max(-1, keepdim=True).values
    den = torch.exp(s - m).sum(-1, keepdim=True)
    p = torch.exp(s - m) / den
    S_p, Rbar = _softmax_scale(p, E(s - m) + S_s)
    S = {"out": torch.einsum("bhij,bhjd->bhid", S_p, vv.abs())}
    S_lse = S["lse"] = (m.abs() + 3 * torch.log(den).abs() + Rbar + 1)[..., 0]
    # backward: p = exp(s - lse) from the saved lse
    S_pb = p * (E(s - ref["lse"][..., None]) + S_s + S_lse[..., None] + 1)
    delta = (gout * ref["out"]).sum(-1, keepdim=True)
    S_delta = (gout.abs() * S["out"]).sum(-1, keepdim=True)
    dp = torch.einsum("bhid,bhjd->bhij", gout, vv)
    S_dp = torch.einsum("bhid,bhjd->bhij", gout.abs(), vv.abs())
    S_ds = S_pb * (dp.abs() + delta.abs()) + p * (S_dp + S_delta)
    S_gq = torch.einsum("bhij,bhjd->bhid", S_ds, kk.abs()) * SCALE
    S_gk = torch.einsum("bhij,bhid->bhjd", S_ds, d["q"].abs() * SCALE)
    S_gv = torch.einsum("bhij,bhid->bhjd", S_pb, gout.abs())
    S["gqkv"] = torch.stack((S_gq, S_gk[:, :, M:], S_gv[:, :, M:]), 1)
    S["gmem"] = torch.stack((S_gk[:, :, :M].sum(0), S_gv[:, :, :M].sum(0))) + (beta * d["gm0"].abs() if beta else 0.0)
    return ref, S


def fa_autograd64(t):
    """float64 autograd of the textbook definition (ddpm.py:265-268 + attend.py) -> out, lse, gqkv, gmem"""
    d = to(t, torch.float64)
    q, k, v, mem = (d[x].clone().requires_grad_(True) for x in ("q", "k", "v", "mem"))
    B = q.shape[0]
    mk, mv = (m.unsqueeze(0).expand(B, -1, -1, -1) for m in mem)
    kk, vv = torch.cat((mk, k), -2), torch.cat((mv, v), -2)
    s = torch.einsum("bhid,bhjd->bhij", q, kk) * SCALE
    out = torch.einsum("bhij,bhjd->bhid", s.softmax(-1), vv)
    out.backward(d["gout"])
    return {"out": out.detach(), "lse": s.logsumexp(-1).detach(), "gqkv": torch.stack((q.grad, k.grad, v.grad), 1),
            "gmem": mem.grad}


# =============================================================================================================================
# one ledger row's operands, float64 results and scales
# =============================================================================================================================
ORDERS = ("torch", "online64", "online128")


class Problem:
    """kind "linattn" | "attn"; geom = (B, heads, H, W, M); ``beta``: the memory gradient is added onto gm0.
    The backward pass of an evaluation reads what ITS forward pass saved, as the kernels do."""

    def __init__(self, kind, geom, family="plain", seed=0, beta=0.0):
        self.kind, self.geom, self.family, self.beta = kind, tuple(geom), family, beta
        la = self.la = kind == "linattn"
        self.t = (la_inputs if la else fa_inputs)(geom, family, seed)
        self.ref, self.S = (la_reference if la else fa_reference)(self.t, beta)
        if not geom[4]:
            self.S.pop("gmem")
        self.tile = LA_TILE if la else FA_TILE

    def _fwd(self, order, mut=None):
        if order == "torch":
            return (la_forward if self.la else fa_forward)(self.t, mut)
        return (la_forward_online if self.la else fa_forward_online)(self.t, int(order[6:]), mut)

    def eval32(self, order):
        f = self._fwd(order)
        f.update((la_backward if self.la else fa_backward)(self.t, f, self.beta))
        return f

    def mutated32(self, mut):
        """the float32 evaluation with one mutation: of the online forward at the kernel's tile (M_ACC, M_WSUM), of the
        backward pass (M_SCALE2, M_RVEC, M_DELTA), else of the forward in torch's order"""
        bmut = mut if mut in (M_SCALE2, M_RVEC, M_DELTA) else None
        f = self._fwd(f"online{self.tile}" if mut in (M_ACC, M_WSUM) else "torch", None if bmut else mut)
        b = (la_backward if self.la else fa_backward)(self.t, f, self.beta, bmut)
        return {**f, **b}


# =============================================================================================================================
# the fused tails of LinearAttention (heads = 4, M = 4): activations are NHWC rows [B * n, channels]
# =============================================================================================================================
def rows_of(x):
    """[B, heads, 32, n] -> [B * n, heads * 32] (channel = head * 32 + d); a leading [B, w, ...] stack -> w * heads * 32"""
    if x.dim() == 5:
        return x.permute(0, 4, 1, 2, 3).reshape(x.shape[0] * x.shape[4], -1)
    return x.permute(0, 3, 1, 2).reshape(x.shape[0] * x.shape[3], -1)


def tail_forward(t, ao):
    """ao [N, hidden] -> o2 = to_out[0](ao) = ao wout^T + bout, y = RMSNorm_g(o2) + x (oracle.norm.rms_forward)"""
    from oracle.norm import rms_forward
    o2 = ao @ t["wout"].t() + t["bout"]
    return {"ao": ao, "o2": o2, "y": rms_forward({"x": o2, "g": t["g"], "res": t["x"]}, True)["y"]}


def tail_forward_scales(d, ref, S_ao):
    """S_o2 = S_ao |wout|^T + |bout|.  y = o2 / ||o2|| g sqrt(C) + x with an o2 that carries S_o2: a change delta of o2
    changes y by (delta - xh <xh, delta>) / ||o2|| g sqrt(C), xh = o2 / ||o2||, so
    S_y = (S_o2 + |xh| sum_c |xh_c| S_o2_c) / ||o2|| |g| sqrt(C) + |x|  (S_o2 >= |o2| makes the second term >= |y - x|: the
    rounding of the norm itself is covered)."""
    S_o2 = S_ao @ d["wout"].abs().t() + d["bout"].abs()
    o2 = ref["o2"]
    nrm = torch.sqrt((o2 * o2).sum(1, keepdim=True)).clamp_min(1e-12)
    xh = (o2 / nrm).abs()
    S_y = (S_o2 + xh * (xh * S_o2).sum(1, keepdim=True)) / nrm * d["g"].abs() * o2.shape[1] ** 0.5 + d["x"].abs()
    return {"ao": S_ao, "o2": S_o2, "y": S_y}


def tail_backward(t, gqkv):
    """gqkv [B, 3, heads, 32, n] -> gxn = G Wqkv [N, C], gw = G^T xn + gw0 [3 hidden, C] (G = the rows of gqkv)"""
    G = rows_of(gqkv)
    return {"gxn": G @ t["wqkv"], "gw": G.t() @ t["xn"] + t["gw0"]}


class TailProblem:
    """kind "la_fwd_tail": lgm_linattn_fwd_fused -> ao, o2, y.  kind "la_bwd_tail": lgm_linattn_bwd_fused from the forward's
    saved ctx / kmax / ksum -> gxn, to_qkv's weight gradient (beta = 1 on gw0) and the memory gradient (beta = 1 on gm0).
    geom = (B, C, H, W); the core's operands are those of la_inputs((B, 4, H, W, 4), family)."""

    def __init__(self, kind, geom, family="plain", seed=0):
        B, C, H, W = geom
        self.kind, self.geom, self.family, self.la, self.tile, self.beta = kind, tuple(geom), family, True, LA_TILE, 1.0
        heads, N = 4, B * H * W
        hidden = heads * DH
        self.t = t = la_inputs((B, heads, H, W, 4), family, seed)
        g = torch.Generator().manual_seed(4000 + seed)
        r = lambda *s: torch.randn(*s, generator=g)
        if kind == "la_fwd_tail":
            t.update(x=r(N, C), wout=r(C, hidden) / hidden ** 0.5, bout=0.1 * r(C), g=1 + 0.2 * r(C))
        else:
            t.update(xn=r(N, C), wqkv=r(3 * hidden, C) * (1.5 / C ** 0.5), gw0=r(3 * hidden, C))
        d = to(t, torch.float64)
        core, S_core = la_reference(t, beta=1.0)
        if kind == "la_fwd_tail":
            self.ref = tail_forward(d, rows_of(core["out"]))
            self.S = tail_forward_scales(d, self.ref, rows_of(S_core["out"]))
            self.ref.update({k: core[k] for k in ("ctx", "kmax", "ksum")})
        else:
            self.ref = dict(tail_backward(d, core["gqkv"]), gmem=core["gmem"])
            SG = rows_of(S_core["gqkv"])
            self.S = {"gxn": SG @ d["wqkv"].abs(), "gw": SG.t() @ d["xn"].abs() + d["gw0"].abs(), "gmem": S_core["gmem"]}

    def _eval(self, order, fmut=None, bmut=None):
        f = la_forward(self.t, fmut) if order == "torch" else la_forward_online(self.t, int(order[6:]), fmut)
        if self.kind == "la_fwd_tail":
            return tail_forward(self.t, rows_of(f["out"]))
        b = la_backward(self.t, f, 1.0, bmut)
        return dict(tail_backward(self.t, b["gqkv"]), gmem=b["gmem"])

    def eval32(self, order):
        return self._eval(order)

    def mutated32(self, mut):
        bmut = mut if mut in (M_SCALE2, M_RVEC) else None
        return self._eval(f"online{self.tile}" if mut in (M_ACC, M_WSUM) else "torch", None if bmut else mut, bmut)
