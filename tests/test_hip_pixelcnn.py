"""The gated PixelCNN prior on the GPU.

Masked convolution kernels (lgm_mconv_xy / _yx / _wgrad): per element against float64 in units of 2^-24 S under
``oracle.bounds.tolerance(n)`` on ``pixelcnn_ref.CONV_SHAPES``, with NaN in every dead weight tap (a kernel that reads one
leaves a NaN), NaN guard lanes around the pitched outputs, causality to the bit, the dead taps of the weight gradient, and
equal bits across two runs and two CU margins.

Gate and cross-entropy against float64 under (k + 2) u M, u = 2^-24, as tests/test_hip_edm.py bounds its elementwise kernels:
M is the sum of the absolute values that enter an element, k the roundings on the way.  A device function counts by its
documented worst error in units of u (tanhf 2 ULP = 4, expf and logf 1 ULP = 2), a correctly rounded operation as 1.
  gate forward  y = x + t s, s = 1 / (1 + e^-b): t 4, s 2 + 1 + 1, the product 1, the sum 1: k = 10, M = |x| + |t s|.
  gate backward ga = (g s)(1 - t^2), gb = (g t)(s (1 - s)): the differences cancel, so M carries their terms:
      M_a = |g| s (1 + t^2), M_b = |g t| s (1 + s); k = 16 covers both (g s 5, t^2 9, the difference 1, the product 1; g t 5,
      s 4, 1 - s 5, two products 2).
  cross-entropy row  loss = (mx + log sum_k e^(l_k - mx)) - l_t: the rounding of l_k - mx enters e relatively, weighted by the
      softmax: D = sum_k p_k |l_k - mx|.  With s = sum_k e^(l_k - mx): M = 1 + |mx| + |log s| + |l_t| + D, k = 16 (expf 2, at most
      K / 64 + 6 <= 14 additions for K <= 512).
  gradient  (e^(l_k - lse) - [k = t]) gloss / M_rows from the kernel's own lse: M = (p (1 + |l_k - lse|) + [k = t]) |gloss / M_rows|,
      k = 6.
  mean: the kernel's own rows summed in float64; k = ceil(rows / 1024) + 23 (a thread's run, the wave tree 6, 16 waves, the
      quotient), M = mean |row|.

Draw, incremental step, the whole network against tests/golden/pixelcnn.npz (tools/make_golden_pixelcnn.py), the VQ-VAE's
``encode_codes`` / ``decode_codes``, the graph-replayed training step and train.py."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pixelcnn_ref as PR
from oracle import bounds

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "pixelcnn.npz")))


@pytest.fixture(scope="module")
def L():
    from lgm_hip import ops
    return ops.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _guarded(dev, lead, C, lo=4, hi=4):
    """A [*lead, C] view with pitch C + lo + hi inside a NaN-filled buffer, and the buffer"""
    buf = torch.full((*lead, C + lo + hi), float("nan"), device=dev)
    return buf[..., lo:lo + C], buf


def _guards_intact(buf, C, lo=4):
    return bool(torch.isnan(buf[..., :lo]).all()) and bool(torch.isnan(buf[..., lo + C:]).all())


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _phys(w, dev, L_live=None, fill=float("nan")):
    """OIHW -> [N][k*k][C] on the device; the dead taps (index >= L_live) hold ``fill``"""
    N, C, k, _ = w.shape
    p = w.permute(0, 2, 3, 1).reshape(N, k * k, C).contiguous().to(dev)
    if L_live is not None:
        p[:, L_live:, :] = fill
    return p


def _geom(B, H, W, C, N, k):
    from lgm_hip import ops
    return ops.make_geom(B, H, W, C, N, k, k, 1, k // 2)


def _within(got, want, mag, k, what, parity):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bound = (k + 2) * U * np.maximum(mag, 1e-300)
    parity(what + f" [worst |err| / ((k + 2) u M), k = {k}]", float((err / bound).max()), 1.0)


# ----------------------------------------------------------------------------------------------------------------------
# masked convolution kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = PR.ConvProblem(shape)
        return cache[shape]
    return get


def _run_mconv(L, dev, p):
    """Every kernel of one layer once -> {kind: result in the layout of ``p.ref[kind]``} and the raw buffers"""
    B, H, W, C, N, k, mt = p.shape
    g, t, Lv = _geom(B, H, W, C, N, k), p.t, p.L
    w = _phys(t["w"], dev, Lv)                                     # NaN in every dead tap
    x, gy, res = _nhwc(t["x"], dev), _nhwc(t["gy"], dev), _nhwc(t["res_x"], dev)
    b = t["b"].to(dev)
    out, raw = {}, {}
    y, ybuf = _guarded(dev, (B, H, W), N)
    L.lgm_mconv_xy(ctypes.byref(g), Lv, x.data_ptr(), C, w.data_ptr(), b.data_ptr(), y.data_ptr(), ybuf.shape[-1], _st())
    assert _guards_intact(ybuf, N), "xy wrote outside its lanes"
    out["xy"] = y.permute(0, 3, 1, 2)
    gx, gxbuf = _guarded(dev, (B, H, W), C)
    L.lgm_mconv_yx(ctypes.byref(g), Lv, gy.data_ptr(), N, w.data_ptr(), res.data_ptr(), C, gx.data_ptr(), gxbuf.shape[-1], _st())
    assert _guards_intact(gxbuf, C), "yx wrote outside its lanes"
    out["yx"] = gx.permute(0, 3, 1, 2)
    for kind, beta in (("wgrad0", 0.0), ("wgrad1", 1.0)):
        if beta:
            gw, gb = _phys(t["gw0"], dev), t["gb0"].to(dev).clone()
        else:
            gw, gb = torch.full((N, k * k, C), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
        before = gw.clone()
        need = L.lgm_mconv_wgrad_workspace(ctypes.byref(g), Lv)
        ws = torch.full((max(need // 4, 4),), float("nan"), device=dev)
        L.lgm_mconv_wgrad(ctypes.byref(g), Lv, gy.data_ptr(), N, x.data_ptr(), C, gw.data_ptr(), gb.data_ptr(), beta,
                          ws.data_ptr(), need, _st())
        raw[kind] = (before, gw)
        out[kind] = torch.cat([gw.view(N, k, k, C).permute(0, 3, 1, 2).reshape(-1), gb])
    torch.cuda.synchronize()
    return out, raw


@pytest.mark.parametrize("shape", PR.CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_convolution_kernels_per_element(L, dev, problems, parity, shape):
    p = problems(shape)
    out, raw = _run_mconv(L, dev, p)
    for kind in ("xy", "yx", "wgrad0", "wgrad1"):
        assert bool(torch.isfinite(out[kind]).all()), f"{kind}: a dead tap (NaN) or a guard lane was read"
        parity(f"{kind} [units of 2^-24 S]", p.score(kind, out[kind]), bounds.tolerance(p.n[kind]))
    before, gw = raw["wgrad0"]
    assert bool((gw[:, p.L:, :] == 0).all()), "beta = 0: the dead taps of gw are exact zeros"
    before, gw = raw["wgrad1"]
    assert torch.equal(gw[:, p.L:, :], before[:, p.L:, :]), "beta = 1: the dead taps of gw are left alone"
    # equal bits: a second run, and a run under another CU margin
    again, _ = _run_mconv(L, dev, p)
    prev = L.lgm_cu_margin()
    L.lgm_set_cu_margin(16 if prev != 16 else 0)
    try:
        other, _ = _run_mconv(L, dev, p)
    finally:
        L.lgm_set_cu_margin(prev)
    for kind in out:
        assert torch.equal(out[kind], again[kind]), f"{kind}: two runs differ"
        assert torch.equal(out[kind], other[kind]), f"{kind}: the CU margin changes the bits"


@pytest.mark.parametrize("shape", PR.CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_convolution_is_causal_to_the_bit(L, dev, problems, shape):
    """type A: the output at p does not see the input at any position >= p (raster order); type B: not at any position > p"""
    p = problems(shape)
    B, H, W, C, N, k, mt = p.shape
    g = _geom(B, H, W, C, N, k)
    w = _phys(p.t["w"], dev, p.L)
    b = p.t["b"].to(dev)
    x = _nhwc(p.t["x"], dev)

    def run(inp):
        y = torch.empty((B, H, W, N), device=dev)
        L.lgm_mconv_xy(ctypes.byref(g), p.L, inp.data_ptr(), C, w.data_ptr(), b.data_ptr(), y.data_ptr(), N, _st())
        return y.view(B, H * W, N)
    base = run(x)
    gen = torch.Generator().manual_seed(5)
    for pos in sorted({0, (H * W) // 2, H * W - 1, min(H * W - 1, W + 1)}):
        first = pos if mt == "A" else pos + 1
        x2 = x.clone().view(B, H * W, C)
        x2[:, first:, :] = torch.randn(B, H * W - first, C, generator=gen).to(dev) * 3
        got = run(x2.view(B, H, W, C))
        assert torch.equal(got[:, pos], base[:, pos]), (pos, "the output sees a later input")
        # a position it may see does reach it: itself (B), else its left neighbour, else the one above
        vis = pos if mt == "B" else pos - 1 if pos % W else pos - W if pos >= W else None
        if vis is not None:
            x3 = x.clone().view(B, H * W, C)
            x3[:, vis, :] += 1.0
            assert not torch.equal(run(x3.view(B, H, W, C))[:, pos], base[:, pos]), (pos, "the live taps stop too early")


# ----------------------------------------------------------------------------------------------------------------------
# gate, cross-entropy
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H", [(5, 4), (37, 20), (128, 128)])
def test_gate_forward_and_backward_against_float64(L, dev, parity, M, H):
    g = torch.Generator().manual_seed(M + H)
    x, gy = torch.randn(M, H, generator=g), torch.randn(M, H, generator=g)
    pre = torch.randn(M, 2 * H, generator=g) * 2
    pre[0, 0], pre[0, H] = 9.0, -30.0                                # a saturated tanh, a vanishing sigmoid
    xd, pd, gd = x.to(dev), pre.to(dev), gy.to(dev)
    y, ybuf = _guarded(dev, (M,), H)
    L.lgm_gated_fwd(xd.data_ptr(), H, pd.data_ptr(), 2 * H, M, H, y.data_ptr(), ybuf.shape[-1], _st())
    assert _guards_intact(ybuf, H)
    a, b = pre[:, :H].double().numpy(), pre[:, H:].double().numpy()
    t, s = np.tanh(a), 1 / (1 + np.exp(-b))
    _within(y.cpu().numpy(), x.double().numpy() + t * s, np.abs(x.double().numpy()) + np.abs(t * s), 10, "gate forward", parity)
    gx0 = torch.randn(M, H, generator=g)
    gx = gx0.to(dev).clone()
    gp, gpbuf = _guarded(dev, (M,), 2 * H)
    L.lgm_gated_bwd(gd.data_ptr(), H, pd.data_ptr(), 2 * H, M, H, gx.data_ptr(), H, gp.data_ptr(), gpbuf.shape[-1], _st())
    assert _guards_intact(gpbuf, 2 * H)
    g64 = gy.double().numpy()
    _within(gp[:, :H].cpu().numpy(), g64 * s * (1 - t * t), np.abs(g64) * s * (1 + t * t), 16, "gate backward: ga", parity)
    _within(gp[:, H:].cpu().numpy(), g64 * t * s * (1 - s), np.abs(g64 * t) * s * (1 + s), 16, "gate backward: gb", parity)
    assert torch.equal(gx.cpu(), gx0 + gy), "gx accumulates gy (one rounding)"
    # over the saved pre-activation, without gx: the same bits
    inplace = pd.clone()
    L.lgm_gated_bwd(gd.data_ptr(), H, inplace.data_ptr(), 2 * H, M, H, None, 0, inplace.data_ptr(), 2 * H, _st())
    assert torch.equal(inplace, gp)


def _xent_case(K, M, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(M, K, generator=g) * 3
    target = torch.randint(0, K, (M,), generator=g)
    logits[1] = logits[1] - logits[1].max() + 80.0                  # a row whose largest logit is 80 ...
    logits[1, K - 1] = logits[1].max() - 7.0
    target[1] = K - 1                                               # ... and whose target is the last class
    target[2] = int(logits[2].argmin())                             # the least likely class
    return logits, target


@pytest.mark.parametrize("K", [5, 12, 512])
def test_cross_entropy_against_float64(L, dev, parity, K):
    M = 2100 if K == 12 else 67                                     # more rows than the mean's 1024 threads, once
    logits, target = _xent_case(K, M, 40 + K)
    pitch = (K + 3) // 4 * 4 + 4
    buf = torch.full((M, pitch), float("nan"), device=dev)
    buf[:, :K] = logits.to(dev)
    td = target.to(dev)
    rows = torch.empty((2, M), device=dev)
    mean = torch.empty(1, device=dev)
    L.lgm_softmax_xent_fwd(buf.data_ptr(), pitch, td.data_ptr(), M, K, rows[0].data_ptr(), rows[1].data_ptr(), mean.data_ptr(),
                           _st())
    l64 = logits.double().numpy()
    mx = l64.max(1)
    e = np.exp(l64 - mx[:, None])
    s = e.sum(1)
    lt = l64[np.arange(M), target.numpy()]
    D = (e / s[:, None] * np.abs(l64 - mx[:, None])).sum(1)
    mag = 1 + np.abs(mx) + np.abs(np.log(s)) + np.abs(lt) + D
    _within(rows[1].cpu().numpy(), mx + np.log(s), mag, 16, f"K = {K}: log-sum-exp", parity)
    _within(rows[0].cpu().numpy(), mx + np.log(s) - lt, mag, 16, f"K = {K}: per-row loss", parity)
    own = rows[0].double().cpu().numpy()
    _within(mean.cpu().numpy(), np.asarray([own.mean()]), np.asarray([np.abs(own).mean()]), math.ceil(M / 1024) + 23,
            f"K = {K}: mean of the kernel's rows", parity)
    parity(f"K = {K}: mean against torch's float64 cross_entropy",
           abs(float(mean) - float(torch.nn.functional.cross_entropy(logits.double(), target))) / float(own.mean()), RTOL)
    # backward from the kernel's own lse
    gloss = torch.tensor([0.7], device=dev)
    lanes = (K + 3) // 4 * 4
    out, obuf = _guarded(dev, (M,), lanes)
    L.lgm_softmax_xent_bwd(buf.data_ptr(), pitch, td.data_ptr(), rows[1].data_ptr(), gloss.data_ptr(), M, K, lanes,
                           out.data_ptr(), obuf.shape[-1], _st())
    assert _guards_intact(obuf, lanes)
    assert bool((out[:, K:] == 0).all()), "pad lanes are zero"
    lse = rows[1].double().cpu().numpy()
    pk = np.exp(l64 - lse[:, None])
    hot = np.zeros_like(pk)
    hot[np.arange(M), target.numpy()] = 1
    scale = float(np.float32(0.7)) / M
    _within(out[:, :K].cpu().numpy(), (pk - hot) * scale, (pk * (1 + np.abs(l64 - lse[:, None])) + hot) * abs(scale), 6,
            f"K = {K}: gradient", parity)


# ----------------------------------------------------------------------------------------------------------------------
# draw
# ----------------------------------------------------------------------------------------------------------------------
def _margin_u(prob64, gen, p_min=1e-3):
    """per row a class with probability > p_min and a u inside it, >= 1e-4 from every boundary -> (classes, u float32)"""
    cdf = np.cumsum(prob64, axis=1)
    cls, us = [], []
    for r in range(prob64.shape[0]):
        ok = np.nonzero(prob64[r] > p_min)[0]
        c = int(ok[int(torch.randint(0, len(ok), (1,), generator=gen))])
        f = 0.1 + 0.8 * float(torch.rand(1, generator=gen))
        u = np.float32((cdf[r, c - 1] if c else 0.0) + f * prob64[r, c])
        assert np.abs(cdf[r] - float(u)).min() >= 1e-4
        cls.append(c)
        us.append(u)
    return np.asarray(cls), torch.tensor(np.asarray(us))


def _draw(L, dev, logits, u, temperature=1.0, codebook=None, C=4, HW=6, p=3):
    B, K = logits.shape
    pitch = (K + 3) // 4 * 4
    lb = torch.full((B, pitch), float("nan"), device=dev)
    lb[:, :K] = logits.to(dev)
    counter = torch.tensor([p], dtype=torch.int32, device=dev)
    codes = torch.full((B, HW), -1, dtype=torch.long, device=dev)
    xin = torch.full((B, HW, C + 4), 7.0, device=dev)
    ud = u.to(dev)
    cb = None if codebook is None else codebook.to(dev).contiguous()
    L.lgm_categorical_draw(lb.data_ptr(), pitch, B, K, temperature, ud.data_ptr(), None if cb is None else cb.data_ptr(),
                           0 if cb is None else cb.shape[1], C, HW, counter.data_ptr(), codes.data_ptr(), xin.data_ptr(), C + 4,
                           1, _st())
    assert counter.tolist() == [p + 1], "the counter advances behind the launch"
    other = [q for q in range(HW) if q != p]
    assert bool((codes[:, other] == -1).all()) and bool((xin[:, other] == 7.0).all()) and bool((xin[:, p, C:] == 7.0).all())
    idx = codes[:, p].cpu()
    want = cb[idx.to(dev)][:, :C] if cb is not None else idx.float().to(dev).unsqueeze(1).expand(B, C)
    assert torch.equal(xin[:, p, :C], want), "the input cache receives the codebook row / the index in every lane"
    return idx.numpy()


@pytest.mark.parametrize("K", [5, 512])
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_draw_is_exact_on_margin_built_uniforms(L, dev, K, temperature):
    g = torch.Generator().manual_seed(K)
    B = 64
    logits = torch.randn(B, K, generator=g) * 2
    prob = torch.softmax(logits.double() / temperature, dim=1).numpy()
    cls, u = _margin_u(prob, g)
    cb = torch.randn(K, 8, generator=g)
    assert _draw(L, dev, logits, u, temperature, codebook=cb, C=8).tolist() == cls.tolist()
    assert _draw(L, dev, logits, u, temperature).tolist() == cls.tolist()
    assert PR.draw(logits, u, temperature).tolist() == cls.tolist(), "the restatement agrees"


@pytest.mark.parametrize("K", [5, 512])
def test_draw_at_the_ends_of_the_unit_interval_and_with_an_impossible_class(L, dev, K):
    g = torch.Generator().manual_seed(3 * K)
    B = 16
    logits = torch.randn(B, K, generator=g)
    logits[:, K - 1] += math.log(K)                                  # the last class holds well over 1e-3 of the mass
    logits[:, 0] += math.log(K)
    zero, top = torch.zeros(B), torch.full((B,), float(np.nextafter(np.float32(1), np.float32(0))))
    assert _draw(L, dev, logits, zero).tolist() == [0] * B
    assert _draw(L, dev, logits, top).tolist() == [K - 1] * B
    dead = logits.clone()
    dead[:, K - 1] = float("-inf")                                   # an impossible last class ...
    dead[:, 0] = float("-inf")                                       # ... and an impossible first one
    dead[:, K - 2] += math.log(K)
    dead[:, 1] += math.log(K)
    assert _draw(L, dev, dead, zero).tolist() == [1] * B, "u = 0 draws the first class with p > 0"
    assert _draw(L, dev, dead, top).tolist() == [K - 2] * B, "the draw is clamped to the last class with p > 0"
    prob = torch.softmax(dead.double(), dim=1).numpy()
    cls, u = _margin_u(prob, g)
    assert _draw(L, dev, dead, u).tolist() == cls.tolist()


# ----------------------------------------------------------------------------------------------------------------------
# incremental step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,N,k,mt,gate", [(3, 5, 6, 8, 16, 7, "A", 0), (5, 4, 7, 16, 32, 7, "B", 1),
                                                  (70, 3, 3, 128, 256, 7, "B", 1), (33, 3, 4, 16, 12, 1, "B", 0)])
def test_incremental_step_per_element_at_corner_edge_and_interior(L, dev, parity, B, H, W, C, N, k, mt, gate):
    g = torch.Generator().manual_seed(B + N)
    T, Lv = k * k, PR.live_taps(k, mt)
    cache = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(N, T, C, generator=g) / math.sqrt(Lv * C)
    bias = torch.randn(N, generator=g)
    wd = w.to(dev).clone()
    wd[:, Lv:, :] = float("nan")
    cd, bd = cache.to(dev), bias.to(dev)
    geom = _geom(B, H, W, C, N, k)
    need = L.lgm_pixelcnn_step_workspace(ctypes.byref(geom), Lv)
    ws = torch.full((need // 4,), float("nan"), device=dev)
    lanes = N // 2 if gate else N
    for pos in sorted({0, W - 1, (H // 2) * W, (H // 2) * W + W // 2, H * W - 1}):
        i, j = divmod(pos, W)
        ref, S = torch.zeros(B, N, dtype=torch.float64), torch.zeros(B, N, dtype=torch.float64)
        for t in range(Lv):
            ih, iw = i + t // k - k // 2, j + t % k - k // 2
            if 0 <= ih < H and 0 <= iw < W:
                ref += cache[:, ih, iw].double() @ w[:, t].double().T
                S += cache[:, ih, iw].double().abs() @ w[:, t].double().abs().T
        ref, S = ref + bias.double(), S + bias.double().abs()
        counter = torch.tensor([pos], dtype=torch.int32, device=dev)
        for at_p in (0, 1):
            lead = (B, H * W) if at_p else (B,)
            out, obuf = _guarded(dev, lead, lanes)
            L.lgm_pixelcnn_step(ctypes.byref(geom), Lv, gate, cd.data_ptr(), C, wd.data_ptr(), bd.data_ptr(), counter.data_ptr(),
                                out.data_ptr(), obuf.shape[-1], at_p, ws.data_ptr(), need, _st())
            assert counter.tolist() == [pos]
            got = out[:, pos] if at_p else out
            if at_p:
                rest = [q for q in range(H * W) if q != pos]
                assert bool(torch.isnan(obuf[:, rest]).all()) and _guards_intact(obuf[:, pos], lanes)
            else:
                assert _guards_intact(obuf, lanes)
            if not gate:
                parity(f"p = {pos}, at_p = {at_p} [units of 2^-24 S]", bounds.forward_error_units(got, ref, S),
                       bounds.tolerance(Lv * C))
            else:
                # the gate magnifies the pre-activations' error by at most |d/da| <= 1, |d/db| <= 1/4: bounded in absolute terms
                a, b = ref[:, :lanes], ref[:, lanes:]
                want = cache[:, i, j, :lanes].double() + torch.tanh(a) * torch.sigmoid(b)
                tol = bounds.tolerance(Lv * C) * U * (S[:, :lanes] + S[:, lanes:]) + 12 * U * (cache[:, i, j, :lanes].abs() + 1)
                assert bool(torch.isfinite(got).all())
                parity(f"p = {pos}, at_p = {at_p}, gated [|err| / bound]", float(((got.double().cpu() - want).abs() / tol).max()),
                       1.0)
    # outside the map nothing is written
    counter = torch.tensor([H * W], dtype=torch.int32, device=dev)
    out, obuf = _guarded(dev, (B, H * W), lanes)
    L.lgm_pixelcnn_step(ctypes.byref(geom), Lv, gate, cd.data_ptr(), C, wd.data_ptr(), bd.data_ptr(), counter.data_ptr(),
                        out.data_ptr(), obuf.shape[-1], 1, ws.data_ptr(), need, _st())
    assert bool(torch.isnan(obuf).all())


# ----------------------------------------------------------------------------------------------------------------------
# the whole network
# ----------------------------------------------------------------------------------------------------------------------
def _weights(fx):
    return PR.init(int(fx["cin"]), int(fx["hid"]), int(fx["K"]), int(fx["layers"]), int(fx["seed"]))


def _net(fx, dev, **kw):
    from models.generative.autoregressive.pixelcnn import PixelCNN
    net = PixelCNN(int(fx["cin"]), int(fx["hid"]), int(fx["K"]), num_layers=int(fx["layers"]), **kw)
    net.load_state_dict(_weights(fx), strict=True)
    net.to(dev)
    net.prepare_hip(dev)
    return net


@pytest.mark.parametrize("route", ["generic", "masked"])
def test_logits_loss_and_live_tap_gradients_against_the_fixture(fx, dev, parity, monkeypatch, route):
    """``route``: the backward's kernels (``MaskedConv2d.backward_route``) - the generic pair on the zero-masked weights (the
    default) and the live-tap pair; the dead taps' gradient is an exact zero on both"""
    from models.generative.autoregressive.pixelcnn import MaskedConv2d
    assert MaskedConv2d.backward_route == "generic"
    monkeypatch.setattr(MaskedConv2d, "backward_route", route)
    net = _net(fx, dev)
    x, target = torch.tensor(fx["x"]).to(dev), torch.tensor(fx["target"]).to(dev)
    with torch.no_grad():
        logits = net(x)
    parity("logits against float64", rel(logits, fx["logits64"]), RTOL)
    parity("logits against the reference's float32", rel(logits, fx["logits"]), RTOL)
    net.train()
    loss = net.training_step((x, target), 0)
    loss.backward()
    parity("loss against float64", abs(float(loss) - float(fx["loss64"])) / float(fx["loss64"]), RTOL)
    # every element of every gradient against the float64 restatement's autograd; the restatement against the fixture
    P64 = {k: v.double().requires_grad_(not k.endswith(".mask")) for k, v in _weights(fx).items()}
    PR.loss(P64, x.double().cpu(), target.cpu()).backward()
    for n, p in net.named_parameters():
        got = p.grad.detach().cpu()
        mask = P64.get(n.replace(".weight", ".mask")) if n.endswith(".weight") else None
        if mask is not None:
            assert bool((got[mask == 0] == 0).all()), f"{n}: the gradient of a dead tap is zero"
            live, ref_live = got[mask > 0], P64[n].grad[mask > 0]
        else:
            live, ref_live = got.reshape(-1), P64[n].grad.reshape(-1)
        parity(f"grad {n} (live taps) against float64", rel(live, ref_live), RTOL)
        if f"grad:{n}" in fx:
            parity(f"grad {n} against the reference's float32", rel(live, fx[f"grad:{n}"]), RTOL)
        else:
            step = live.numel() // int(fx["grad_sample"])
            parity(f"grad {n}: norm against the reference's", abs(float(live.double().norm()) - float(fx[f"gradnorm:{n}"]))
                   / float(fx[f"gradnorm:{n}"]), RTOL)
            parity(f"grad {n}: sample against the reference's", rel(live[::step][:int(fx["grad_sample"])], fx[f"gradsample:{n}"]),
                   RTOL)


def _chain(net, fx, dev, capture):
    from models.generative.autoregressive.pixelcnn import _PixelChain
    net.grid = (int(fx["H"]), int(fx["W"]))
    cb = torch.tensor(fx["codebook"]).to(dev).contiguous()
    return _PixelChain(net, int(fx["B"]), 1.0, cb.data_ptr(), capture=capture), cb


def test_sampled_chain_draws_the_fixtures_codes_eager_and_replayed(fx, dev):
    net = _net(fx, dev)
    u = torch.tensor(fx["uniforms"])
    eager, cb = _chain(net, fx, dev, False)
    codes_e, xin_e = eager.run(u)
    assert torch.equal(codes_e.cpu(), torch.tensor(fx["codes"])), "every position, no exception"
    graphed, cb2 = _chain(net, fx, dev, True)
    assert graphed.graphs is not None
    codes_g, xin_g = graphed.run(u)
    assert torch.equal(codes_g, codes_e) and torch.equal(xin_g, xin_e)
    assert torch.equal(graphed.logits, eager.logits), "eager launches and graph replay give the same bits"
    assert torch.equal(xin_e[..., :cb.shape[1]], cb[codes_e]), "the input cache holds the drawn codes' rows"
    again, _ = graphed.run(u)
    assert torch.equal(again, codes_g), "a second run starts from a clean cache"
    drawn, _ = graphed.run(None)                                   # uniforms drawn inside the graph
    assert drawn.min() >= 0 and drawn.max() < int(fx["K"])


def test_incremental_logits_equal_the_full_forward_at_every_position(fx, dev, parity):
    net = _net(fx, dev)
    chain, cb = _chain(net, fx, dev, False)
    u = torch.tensor(fx["uniforms"]).to(dev)
    H, W, K = int(fx["H"]), int(fx["W"]), int(fx["K"])
    chain.xin.zero_()
    chain.counter.zero_()
    chain.inject = True
    seen = []
    for p in range(H * W):
        chain.u.copy_(u[p])
        chain.one_step()
        seen.append(chain.logits[:, :K].clone())
    codes = chain.codes.view(-1, H, W)
    assert torch.equal(codes.cpu(), torch.tensor(fx["codes"]))
    with torch.no_grad():
        full = net(cb[codes].permute(0, 3, 1, 2).contiguous())       # [B, K, H, W]
    P64 = {k: v.double() for k, v in _weights(fx).items()}
    _, ref64 = PR.chain(P64, torch.tensor(fx["codebook"]).double(), torch.tensor(fx["uniforms"]), H, W)
    worst = max(rel(seen[p], full[:, :, p // W, p % W]) for p in range(H * W))
    parity("incremental logits against the full forward, worst position", worst, RTOL)
    parity("incremental logits against the float64 chain, worst position", max(rel(seen[p], ref64[p]) for p in range(H * W)), RTOL)


# (lgm_vq_assign takes embedding dimensions 16 / 32 / 64 / 128)
VQ_ARGS = dict(img_channels=3, img_size=16, embedding_dim=16, num_embeddings=12, hidden_dim=16, num_residual_layers=1,
               num_residual_hiddens=8)


def _vqvae(dev, seed=11):
    from models.generative.vae.vqvae import VQVAE
    torch.manual_seed(seed)
    vq = VQVAE(**VQ_ARGS)
    vq.to(dev)
    vq.prepare_hip(dev).data.mul_(3.0)
    vq.eval()
    with torch.no_grad():                                            # the codebook: latents of three images, so codes vary
        x0 = torch.rand(3, 3, 16, 16, generator=torch.Generator().manual_seed(seed)).to(dev) * 2 - 1
        lat = vq.run(x0, False)[0]["latents"]
        vq.vector_quantizer.embedding.weight.copy_(lat.reshape(12, 16))
    return vq


def test_vqvae_decode_codes_of_encode_codes_is_its_own_reconstruction(dev):
    vq = _vqvae(dev)
    x = torch.rand(5, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev) * 2 - 1
    ema = vq.vector_quantizer._ema_cluster_size.clone()
    with torch.no_grad():
        xh, _, _ = vq(x)
        idx = vq.encode_codes(x)
        out = vq.decode_codes(idx)
    assert idx.dtype == torch.long and tuple(idx.shape) == (5, 2, 2) and len(set(idx.reshape(-1).tolist())) > 1
    assert torch.equal(out, xh), "decode_codes(encode_codes(x)) is x_hat to the bit"
    vq.train()
    vq.encode_codes(x)
    assert torch.equal(vq.vector_quantizer._ema_cluster_size, ema), "encoding never updates the EMA codebook"


def test_sample_with_and_without_a_vqvae(fx, dev, monkeypatch):
    from lgm_hip import captured
    from models.generative.autoregressive.pixelcnn import PixelCNN
    vq = _vqvae(dev)
    torch.manual_seed(5)
    net = PixelCNN(16, 16, 12, num_layers=2, vqvae=vq, img_size=16, img_channels=3)
    net.to(dev)
    u = torch.rand(4, 6, generator=torch.Generator().manual_seed(2))
    imgs, codes = net.sample(6, uniforms=u, return_codes=True)
    assert tuple(imgs.shape) == (6, 3, 16, 16) and bool(torch.isfinite(imgs).all()) and float(imgs.abs().max()) <= 1.0
    assert tuple(codes.shape) == (6, 2, 2) and codes.dtype == torch.long and 0 <= int(codes.min()) and int(codes.max()) < 12
    keys = list(captured._GRAPHS[net])
    assert keys and all(k[0] == "pixelcnn" for k in keys) and not isinstance(captured._GRAPHS[net][keys[0]], int)
    assert torch.equal(net.sample(6, uniforms=u), imgs)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager, codes_e = net.sample(6, uniforms=u, return_codes=True)
    monkeypatch.delenv("LGM_NO_SAMPLER_GRAPH")
    assert torch.equal(codes_e, codes) and torch.equal(eager, imgs), "eager launches and graph replay give the same bits"
    sharp, cs = net.sample(6, temperature=0.05, uniforms=u, return_codes=True)
    assert tuple(cs.shape) == (6, 2, 2)
    with pytest.raises(ValueError, match="uniforms"):
        net.sample(6, uniforms=u[:3])
    assert tuple(net.sample(3).shape) == (3, 3, 16, 16)
    # without a VQ-VAE: the reference's semantics, the index as a float in every channel
    plain = _net(fx, dev, img_size=3)
    out, codes = plain.sample(4, return_codes=True)
    assert tuple(out.shape) == (4, int(fx["cin"]), 3, 3)
    assert torch.equal(out, codes.float().unsqueeze(1).expand_as(out))


def test_three_fast_steps_equal_forward_backward_and_the_same_optimizer(fx, dev):
    a, b = _net(fx, dev), _net(fx, dev)
    a.train(), b.train()
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa = a.make_fast_step(oa, 1, True)
    g = torch.Generator().manual_seed(9)
    B, C, H, W, K = 4, int(fx["cin"]), int(fx["H"]), int(fx["W"]), int(fx["K"])
    batches = [(torch.randn(B, C, H, W, generator=g).to(dev), torch.randint(0, K, (B, H, W), generator=g).to(dev))
               for _ in range(3)]
    la = [fa.step((x.clone(), t.clone()), i).detach().clone().reshape(()) for i, (x, t) in enumerate(batches)]
    assert fa.mode.startswith("hipGraph"), fa.mode
    lb = []
    for i, (x, t) in enumerate(batches):
        loss = b.training_step((x, t), i)
        loss.backward()
        ob.step()
        ob.zero_grad()
        lb.append(loss.detach().clone().reshape(()))
    assert all(torch.equal(p, q) for p, q in zip(la, lb)), (la, lb)
    assert torch.equal(a._flat.data, b._flat.data)
    assert float(la[0]) != float(la[2])
    for n, p in a.state_dict().items():
        if n.endswith(".mask"):
            assert bool((a.state_dict()[n.replace(".mask", ".weight")][p == 0] == 0).all()), "Adam leaves the dead taps at zero"


def test_train_entry_trains_the_prior_over_a_checkpointed_vqvae(dev, tmp_path):
    """train.py's main() on configs/vae/vqvae_prior.json at a reduced size (16 x 16 images, a 2 x 2 grid): the VQ-VAE comes
    from ``vqvae.ckpt_path``, a few graph-replayed steps, and the checkpoint carries it under ``vqvae.*``"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    vq = _vqvae(dev)
    vq_sd = {k: v.detach().cpu().clone() for k, v in vq.state_dict().items()}
    torch.save({"state_dict": vq_sd}, tmp_path / "vqvae.ckpt")
    cfg = json.load(open(os.path.join(pkg, "configs", "vae", "vqvae_prior.json")))
    cfg["dataset"].update(img_size=16, batch_size=8)
    cfg["model"]["args"].update(img_size=16, input_channels=16, output_channels=12, hidden_channels=16, num_layers=2,
                                vqvae={"args": VQ_ARGS, "ckpt_path": str(tmp_path / "vqvae.ckpt")})
    path = tmp_path / "prior_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_vqvae_prior"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('STEPS', m.global_step, m.trainer.fast.mode); print('TRAIN_LOSS', float(m.logged['train_loss'])); "
            "s = m.sample(3); print('SAMPLES', tuple(s.shape), bool(torch.isfinite(s).all()))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "4", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "TRAIN_LOSS", "SAMPLES"))}
    assert lines["STEPS"].startswith("STEPS 4 hipGraph replay"), lines
    loss = float(lines["TRAIN_LOSS"].split()[1])
    assert np.isfinite(loss) and loss < 2 * math.log(12)
    assert lines["SAMPLES"] == "SAMPLES (3, 3, 16, 16) True", lines
    sd = torch.load(os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt"), map_location="cpu",
                    weights_only=False)
    assert sd["global_step"] == 4
    for k, v in vq_sd.items():
        assert torch.equal(sd["state_dict"][f"vqvae.{k}"], v), f"the frozen VQ-VAE changed: {k}"
