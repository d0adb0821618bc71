"""The denoising autoencoder on the GPU (csrc/dae.hip, ReLU in csrc/dense.hip, models/generative/autoencoder/dae.py).

Dense kernels with ReLU (lgm_dense_fwd / lgm_dense_bwd / lgm_dense_dgrad): per element against float64 in units of 2^-24 S
under ``oracle.bounds.tolerance(n)``, n = K forward, N for the input gradient, B for the weight and bias gradients, on
``vae_ref.DENSE_SHAPES`` with the operands of ``oracle.bounds.Problem`` (bias on, beta = 1 on a previous gw / gb).
tests/test_dae_host.py shows that the reference's own float32 stays under C_REF_WORST on these shapes with ReLU.  ReLU is
1-Lipschitz, so the forward bound of the pre-activation holds for the output; the backward reads its mask from a saved
output that is 0 or >= 1e-3.  NaN sits in every pad lane and padding row of the weights, of their transposed copy and of the
bias, and in the pad lanes of the inputs; NaN guard lanes surround every output and must stay NaN; pad lanes of outputs must
be exactly 0.  Equal bits on a second run, from the scalar-load form of an unaligned input, and at CU margins 0 and 16.

lgm_dae_corrupt: two correctly rounded operations in torch's order - equal bits with the CPU's float32 x + noise * level.
lgm_dae_corrupt_mask: no arithmetic - equal bits with the numpy restatement (tests/dae_ref.py), x's bits where untouched.

Head and loss against float64 under (k + 2) u M, u = 2^-24, as tests/test_hip_vae.py bounds its elementwise kernels: M is the
sum of the absolute values that enter an element, k the roundings on the way.  tanhf counts by its
documented worst error of 2 ULP = 4 u, a correctly rounded operation as 1.
  x_hat           tanhf: k = 4.
  row_part        from the kernel's own x_hat: per term the difference 1 (twice, squared) and the square 1: 3; a thread adds
                  the 4 elements of a quad and ceil(D / 1024) quads: 4 ceil(D / 1024) additions, the wave tree 6, four waves
                  4: k = 13 + 4 ceil(D / 1024), M = sum (x - x_hat)^2.
  gpre            c = 2 gloss / (B D): the doubling is exact, the quotient 1; the difference 1; c (x_hat - x) 1; x_hat^2 1;
                  1 - x_hat^2 1 (M carries 1 + x_hat^2); the product 1: k = 6, M = |c| |x_hat - x| (1 + x_hat^2); exactly 0
                  where x_hat == x.
  loss            from the kernel's own partials: ceil(B / 64) additions per lane, the tree 6, the quotient 1.

The whole network against tests/golden/dae.npz (tools/make_golden_dae.py) at the project's 1e-4 on both routes of
``lgm_hip.nn.Linear``, the float64 restatement at an unaligned D = 75, the graph-replayed step against eager launches to the
bit, the no-tape paths to the bit, and train.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dae_ref as DR
import vae_ref as VR
from oracle import bounds

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24
NAN = float("nan")
ACT_NONE, ACT_RELU = 0, 3
EW_SHAPES = [(1, 1), (3, 75), (4, 64), (5, 784), (33, 260)]
KEYS64 = (0x0123_4567_89AB_CDEF, -3, 5)     # a non-zero high half, a negative key, a zero high half


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dae.npz")))


def _ops():
    from lgm_hip import ops
    return ops


def _r4(n):
    return (n + 3) // 4 * 4


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a.reshape(-1) - b.reshape(-1)).norm() / b.norm().clamp_min(1e-30))


def _guarded(dev, B, C, lo=4, hi=4):
    """A [B, C] view with pitch C + lo + hi inside a NaN-filled buffer, and the buffer"""
    buf = torch.full((B, C + lo + hi), NAN, device=dev)
    return buf[:, lo:lo + C], buf


def _guards_intact(buf, C, lo=4):
    return bool(torch.isnan(buf[:, :lo]).all()) and bool(torch.isnan(buf[:, lo + C:]).all())


def _flat_guarded(dev, n):
    buf = torch.full((n + 8,), NAN, device=dev)
    return buf[4:4 + n], buf


def _flat_guards_intact(buf):
    return bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[-4:]).all())


def _phys(w2, dev, fill=NAN):
    """[N, K] -> FlatParams' [Np][Kp] on the device; pad lanes and padding rows hold ``fill``"""
    N, K = w2.shape
    p = torch.full((_r4(N), _r4(K)), fill)
    p[:N, :K] = w2
    return p.to(dev)


def _vec(v, dev, fill=NAN):
    p = torch.full((_r4(v.numel()),), fill)
    p[:v.numel()] = v
    return p.to(dev)


def _input(a2, dev):
    """[B, C] -> (a view with a padded pitch on a 16-byte aligned base and NaN pad lanes: the 16-byte-load form;
    a view of the same values on a base 4 bytes off: the scalar-load form)"""
    B, C = a2.shape
    v, _ = _guarded(dev, B, _r4(C))
    v[:, :C] = a2.to(dev)
    off = torch.empty(B * C + 1, device=dev)[1:].view(B, C)
    off.copy_(a2.to(dev))
    return v[:, :C], off


def _margins(L, run):
    """``run()`` at CU margins 0 and 16 -> the two results"""
    out = []
    try:
        for m in (0, 16):
            L.lgm_set_cu_margin(m)
            out.append(run())
    finally:
        L.lgm_set_cu_margin(-1)
    return out


def _within(got, want, mag, k, what, parity):
    err = np.abs(np.asarray(torch.as_tensor(got).detach().double().cpu()) - np.asarray(want))
    bound = (k + 2) * U * np.maximum(np.asarray(mag), 1e-300)
    parity(what + f" [worst |err| / ((k + 2) u M), k = {k}]", float((err / bound).max()), 1.0)


_ids = lambda s: "x".join(map(str, s))      # noqa: E731


# ----------------------------------------------------------------------------------------------------------------------
# dense kernels with ReLU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VR.DENSE_SHAPES, ids=_ids)
def test_dense_forward_relu_per_element(dev, parity, shape):
    ops = _ops()
    L = ops.lib()
    B, K, N = shape
    t = bounds.Problem("xy", (B, 1, 1, K, N, 1, 1, 0)).t
    x, w, b = t["x"].view(B, K), t["w"].view(N, K), t["b"]
    pre = x.double() @ w.double().T + b.double()
    S = x.abs().double() @ w.abs().double().T + b.abs().double()
    wd, bd = _phys(w, dev), _vec(b, dev)
    xv, xo = _input(x, dev)
    Np = _r4(N)

    def run(xin):
        yv, ybuf = _guarded(dev, B, Np)
        ops.dense_fwd(xin, wd.data_ptr(), bd.data_ptr(), K, N, yv, ACT_RELU, 0.0)
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, Np), "guard lanes written"
        return yv.clone()

    y = run(xv)
    parity(f"dense_fwd {_ids(shape)} relu [units of 2^-24 S]", bounds.forward_error_units(y[:, :N], torch.relu(pre), S),
           bounds.tolerance(K))
    assert bool((y >= 0).all()) and not bool(torch.signbit(y).any()), "the clamped side is +0"
    assert int((y[:, :N] == 0).sum()) > 0 and int((y[:, :N] > 0).sum()) > 0, "both sides of the kink occur"
    assert bool((y[:, N:] == 0).all()), "pad lanes of the output are exactly 0"
    assert torch.equal(run(xv), y), "a second run gives the same bits"
    assert torch.equal(run(xo), y), "the scalar-load form of the input gives the same bits"
    m0, m16 = _margins(L, lambda: run(xv))
    assert torch.equal(m0, m16), "CU margins 0 and 16 give the same bits"


def _saved_output(B, N):
    """a ReLU layer's saved output: about 40 % exact zeros, the rest >= 1e-3"""
    y0 = torch.randn(B, N, generator=torch.Generator().manual_seed(B + N))
    return torch.where(y0 > -0.25, y0.abs().clamp(max=1.0) + 1e-3, torch.zeros_like(y0))


@pytest.mark.parametrize("shape", VR.DENSE_SHAPES, ids=_ids)
def test_dense_backward_and_dgrad_relu_per_element(dev, parity, shape):
    ops = _ops()
    L = ops.lib()
    B, K, N = shape
    t = bounds.Problem("wgrad", (B, 1, 1, K, N, 1, 1, 0)).t
    x, w, gy = t["x"].view(B, K), t["w"].view(N, K), t["gy"].view(B, N)
    gw0, gb0 = t["gw0"].view(N, K), t["gb0"]
    need_gx = shape != (33, 784, 512)                     # the config's first layer has no input gradient
    y = _saved_output(B, N)
    Np, Kp = _r4(N), _r4(K)
    wt = _phys(w.T.contiguous(), dev)                     # [Kp][Np], NaN in its pad lanes and padding rows
    xv, _ = _input(x, dev)
    gyv, gyo = _input(gy, dev)
    yv, yo = _input(y, dev)

    def run(gyin=gyv, yin=yv):
        gwv, gwbuf = _flat_guarded(dev, Np * Kp)
        gbv, gbbuf = _flat_guarded(dev, Np)
        gwv.zero_(), gbv.zero_()
        gwv.view(Np, Kp)[:N, :K] = gw0.to(dev)
        gbv[:N] = gb0.to(dev)
        gxv, gxbuf = _guarded(dev, B, Kp) if need_gx else (None, None)
        ops.dense_bwd(gyin, yin, xv, wt.data_ptr() if need_gx else None, K, N, gxv, gwv.data_ptr(), gbv.data_ptr(), 1.0,
                      ACT_RELU, 0.0)
        torch.cuda.synchronize()
        assert _flat_guards_intact(gwbuf) and _flat_guards_intact(gbbuf), "guard lanes written"
        assert gxbuf is None or _guards_intact(gxbuf, Kp), "guard lanes written"
        return (gxv.clone() if need_gx else None), gwv.view(Np, Kp).clone(), gbv.clone()

    def dgrad(gyin=gyv, yin=yv):
        gxv, gxbuf = _guarded(dev, B, Kp)
        ops.dense_dgrad(gyin, yin, wt.data_ptr(), K, N, gxv, ACT_RELU, 0.0)
        torch.cuda.synchronize()
        assert _guards_intact(gxbuf, Kp), "guard lanes written"
        return gxv.clone()

    g64 = gy.double() * (y > 0)
    gx, gw, gb = run()
    gx_ref, gx_S = g64 @ w.double(), g64.abs() @ w.abs().double()
    if need_gx:
        parity(f"dense_bwd gx {_ids(shape)} relu [units of 2^-24 S]", bounds.forward_error_units(gx[:, :K], gx_ref, gx_S),
               bounds.tolerance(N))
        assert bool((gx[:, K:] == 0).all()), "pad lanes of gx are exactly 0"
    ref = torch.cat([(gw0.double() + g64.T @ x.double()).reshape(-1), gb0.double() + g64.sum(0)])
    S = torch.cat([(gw0.abs().double() + g64.abs().T @ x.abs().double()).reshape(-1), gb0.abs().double() + g64.abs().sum(0)])
    got = torch.cat([gw[:N, :K].reshape(-1), gb[:N]])
    parity(f"dense_bwd gw, gb {_ids(shape)} relu [units of 2^-24 S]", bounds.forward_error_units(got, ref, S), bounds.tolerance(B))
    assert bool((gw[N:] == 0).all()) and bool((gw[:, K:] == 0).all()) and bool((gb[N:] == 0).all()), "pads stay exactly 0"
    same = lambda a, b_: all(p is None or torch.equal(p, q) for p, q in zip(a, b_))      # noqa: E731
    assert same(run(), (gx, gw, gb)), "a second run gives the same bits"
    assert same(run(gyo, yo), (gx, gw, gb)), "the scalar-load form gives the same bits"
    m0, m16 = _margins(L, run)
    assert same(m0, m16), "CU margins 0 and 16 give the same bits"
    # the input gradient alone
    dg = dgrad()
    parity(f"dense_dgrad {_ids(shape)} relu [units of 2^-24 S]", bounds.forward_error_units(dg[:, :K], gx_ref, gx_S),
           bounds.tolerance(N))
    assert bool((dg[:, K:] == 0).all())
    assert gx is None or torch.equal(dg, gx), "the same bits as lgm_dense_bwd's gx"
    assert torch.equal(dgrad(), dg) and torch.equal(dgrad(gyo, yo), dg)
    d0, d16 = _margins(L, dgrad)
    assert torch.equal(d0, d16)


def test_dense_backward_relu_at_exact_zeros_of_y_follows_torch(dev):
    """ReLU'(0) = 0, torch's choice: with one row and beta = 0 the bias gradient IS g = gy * act'(y)"""
    ops = _ops()
    K, N = 12, 8
    g = torch.Generator().manual_seed(3)
    pre = torch.randn(1, N, generator=g)
    pre[0, ::3] = 0.0
    pre.requires_grad_(True)
    gy, x = torch.randn(1, N, generator=g), torch.randn(1, K, generator=g)
    y = torch.relu(pre)
    y.backward(gy)
    gw = torch.zeros(N, K, device=dev)
    gb = torch.full((N,), NAN, device=dev)                # beta = 0 overwrites whatever is there
    ops.dense_bwd(gy.to(dev), y.detach().to(dev), x.to(dev), None, K, N, None, gw.data_ptr(), gb.data_ptr(), 0.0, ACT_RELU, 0.0)
    assert torch.equal(gb.cpu(), pre.grad[0])
    assert torch.equal(gw.cpu(), pre.grad[0][:, None] * x)          # one product per element: no sum to round


# ----------------------------------------------------------------------------------------------------------------------
# corruption
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", EW_SHAPES)
def test_corrupt_equals_the_cpu_float32_result_to_the_bit(dev, B, D):
    ops = _ops()
    Dp = _r4(D)
    g = torch.Generator().manual_seed(31 * B + D)
    x, noise = torch.rand(B, D, generator=g) * 2 - 1, torch.randn(B, D, generator=g)
    (xa, xo), (na, no) = _input(x, dev), _input(noise, dev)
    for level in (0.0, 0.1, 1.0):
        want = x + noise * level
        for xin, nin in ((xa, na), (xo, no), (xa, no)):       # aligned, 4 bytes off, and one of each
            ov, obuf = _guarded(dev, B, Dp)
            ops.dae_corrupt(xin, nin, level, ov)
            torch.cuda.synchronize()
            assert _guards_intact(obuf, Dp), "guard lanes written"
            assert torch.equal(ov[:, :D].cpu(), want), (level, "x + noise * level, two roundings")
            assert bool((ov[:, D:] == 0).all()) and not bool(torch.signbit(ov[:, D:]).any()), "pad lanes are +0"
    o2 = torch.full((B, Dp), NAN, device=dev)               # an output without a gap between its rows
    ops.dae_corrupt(xa, na, 0.1, o2)
    assert torch.equal(o2[:, :D].cpu(), x + noise * 0.1) and bool((o2[:, D:] == 0).all())


@pytest.mark.parametrize("mode", ["salt_and_pepper", "masking"])
@pytest.mark.parametrize("B,D", EW_SHAPES)
def test_corrupt_mask_equals_the_numpy_restatement(dev, B, D, mode):
    ops = _ops()
    Dp = _r4(D)
    g = torch.Generator().manual_seed(17 * B + D)
    x = torch.rand(B, D, generator=g) * 0.8 + 0.1           # neither 0 nor 1: a hit shows
    x[0, 0] = -0.0                                          # a sign bit survives where nothing hits
    forms = _input(x, dev)
    xb = x.numpy().view(np.uint32)
    for key in KEYS64:
        kd = torch.tensor([key], dtype=torch.int64, device=dev)
        ws, wp = (w.reshape(B, D) for w in DR.mask_words(B * D, key))
        for level in (0.0, 0.1, 1.0, 2.0):
            want = DR.corrupt_mask(x.numpy(), key, mode, level)
            thr = np.uint64(DR.mask_threshold(mode, level))
            untouched = (ws >= thr) & ((wp >= thr) | (mode == "masking"))
            assert untouched.all() if level == 0.0 else not untouched.all() or B * D < 4
            for xin in forms:
                ov, obuf = _guarded(dev, B, Dp)
                ops.dae_corrupt_mask(xin, kd, mode, level, ov)
                torch.cuda.synchronize()
                assert _guards_intact(obuf, Dp), "guard lanes written"
                got = ov[:, :D].cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, level)
                assert np.array_equal(got.view(np.uint32)[untouched], xb[untouched]), "untouched elements keep x's bits"
                assert bool((ov[:, D:] == 0).all()), "pad lanes are exactly 0"
    # the key is read when the kernel runs: refilled in place, the same launch arguments give the other mask
    kd = torch.tensor([KEYS64[0]], dtype=torch.int64, device=dev)
    o1, o2 = torch.empty(B, Dp, device=dev), torch.empty(B, Dp, device=dev)
    ops.dae_corrupt_mask(forms[0], kd, mode, 1.0, o1)
    kd.fill_(KEYS64[1])
    ops.dae_corrupt_mask(forms[0], kd, mode, 1.0, o2)
    assert np.array_equal(o2[:, :D].cpu().numpy(), DR.corrupt_mask(x.numpy(), KEYS64[1], mode, 1.0))
    assert np.array_equal(o1[:, :D].cpu().numpy(), DR.corrupt_mask(x.numpy(), KEYS64[0], mode, 1.0))


# ----------------------------------------------------------------------------------------------------------------------
# tanh + squared error, loss
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", EW_SHAPES + [(512, 260)])
def test_tanh_mse_and_the_loss_against_float64(dev, parity, B, D):
    ops = _ops()
    Dp = _r4(D)
    g = torch.Generator().manual_seed(B * 1000 + D)
    pre = torch.randn(B, D, generator=g) * 1.5
    x = torch.rand(B, D, generator=g) * 2 - 1
    prev, preo = _input(pre, dev)
    x_d = x.to(dev).contiguous()                           # rows of D floats: not 16-byte aligned for D = 1, 75
    tag = f"B{B} D{D}"

    def fwd(pin=prev, xin=None):
        xhv, xbuf = _guarded(dev, B, Dp)
        row = torch.full((B,), NAN, device=dev)
        ops.dae_tanh_mse_fwd(pin, x_d if xin is None else xin, D, xhv, row)
        torch.cuda.synchronize()
        assert _guards_intact(xbuf, Dp)
        return xhv, row
    xh, _ = fwd()
    hit = torch.rand(B, D, generator=g) < 0.1
    hit[0, 0] = True
    x_d[hit.to(dev)] = xh[:, :D][hit.to(dev)]              # exact zeros of x_hat - x
    xh, row = fwd()
    x = x_d.cpu()
    t64 = torch.tanh(pre.double())
    _within(xh[:, :D], t64, t64.abs(), 4, f"x_hat {tag}", parity)
    assert bool((xh[:, D:] == 0).all())
    xh64 = xh[:, :D].double().cpu()
    diff = xh64 - x.double()
    assert int((diff == 0).sum()) >= int(hit.sum())
    sq = (diff ** 2).sum(1)
    _within(row, sq, sq, 13 + 4 * ((D + 1023) // 1024), f"row_part {tag}", parity)
    xh2, row2 = fwd()
    assert torch.equal(xh2[:, :D], xh[:, :D]) and torch.equal(row2, row), "a second run gives the same bits"
    xva, xvo = _input(x, dev)
    for pin, xin in ((preo, xvo), (prev, xva), (preo, xva)):
        xh3, row3 = fwd(pin, xin)
        assert torch.equal(xh3[:, :D], xh[:, :D]) and torch.equal(row3, row), "both load forms give the same bits"

    gloss = torch.tensor([1.3])
    gl_d = gloss.to(dev)

    def bwd(hin, xin):
        gpv, gbuf = _guarded(dev, B, Dp)
        ops.dae_tanh_mse_bwd(hin, xin, gl_d, D, gpv)
        torch.cuda.synchronize()
        assert _guards_intact(gbuf, Dp) and bool((gpv[:, D:] == 0).all())
        return gpv
    gpv = bwd(xh, x_d)
    c = 2.0 * float(gloss[0]) / (B * D)
    _within(gpv[:, :D], c * diff * (1 - xh64 ** 2), abs(c) * diff.abs() * (1 + xh64 ** 2), 6, f"gpre {tag}", parity)
    assert bool((gpv[:, :D][hit.to(dev)] == 0).all()), "exactly 0 where x_hat == x"
    hva, hvo = _input(xh[:, :D].cpu(), dev)
    assert torch.equal(bwd(hvo, xvo)[:, :D], gpv[:, :D]) and torch.equal(bwd(hva, xva)[:, :D], gpv[:, :D])

    vals = torch.full((1,), NAN, device=dev)
    ops.dae_loss(row, D, vals)
    r64 = row.double().cpu()
    _within(vals[0], r64.sum() / (B * D), r64.abs().sum() / (B * D), (B + 63) // 64 + 7, f"loss {tag}", parity)
    v2 = torch.full((1,), NAN, device=dev)
    ops.dae_loss(row, D, v2)
    assert torch.equal(v2, vals)


# ----------------------------------------------------------------------------------------------------------------------
# the whole network
# ----------------------------------------------------------------------------------------------------------------------
def _net(C, S, seed, dev, **kw):
    from models.generative.autoencoder.dae import DAE
    m = DAE(C, S, **kw)
    m.load_state_dict(DR.dae_init(C, S, seed))
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


def _fx_net(fx, case, dev, **kw):
    C, S, B = fx[f"{case}:dims"].tolist()
    return _net(C, S, int(fx[f"{case}:seed"]), dev, noise_type=str(fx[f"{case}:noise_type"]),
                noise_level=float(fx[f"{case}:level"]), **kw)


def _routes(monkeypatch, route):
    from lgm_hip.nn import Linear
    monkeypatch.setattr(Linear, "fwd_route", "generic" if route == "generic" else "dense")
    monkeypatch.setattr(Linear, "bwd_route", "dense" if route == "dense" else "generic")


@pytest.mark.parametrize("route", ["dense", "generic", "generic_bwd"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_whole_network_against_the_reference_fixture(fx, dev, parity, monkeypatch, case, route):
    """every route of ``lgm_hip.nn.Linear`` with ReLU: the dense kernels, the generic 1x1 kernels in both directions, and the
    generic backward alone"""
    _routes(monkeypatch, route)
    m = _fx_net(fx, case, dev)
    C, S, B = fx[f"{case}:dims"].tolist()
    D = C * S * S
    x = torch.from_numpy(fx[f"{case}:x"]).to(dev)
    want_xc = torch.from_numpy(fx[f"{case}:corrupted"])
    if case == "a":                                        # the reference's draw through the corruption kernel: its bits
        xc = m.corrupt(x, noise=torch.from_numpy(fx["a:draws"]).to(dev))
        assert torch.equal(xc.cpu(), want_xc)
    else:                                                  # the reference's mask comes from another generator: the bypass
        xc = want_xc.to(dev)
    (vals, xh), tape = m.run(x, xc.reshape(B, D), True)
    m._flat.zero_grad()
    m.backward_hip(tape, torch.ones(1, device=dev))
    torch.cuda.synchronize()
    parity(f"case {case} {route}: x_hat", rel(xh[:, :D], fx[f"{case}:x_hat"]), RTOL)
    parity(f"case {case} {route}: loss", rel(vals[0], fx[f"{case}:loss"]), RTOL)
    for n, p in m.named_parameters():
        parity(f"case {case} {route}: grad {n}", DR.fixture_grad_error(fx, case, n, p.grad), RTOL)
    grads = m._flat.grad.clone()
    # the same through autograd's one Function and the bypass: the same bits; then with the draw inside: finite
    loss = m.training_step((x, None), 0, corrupted=xc)
    m._flat.zero_grad()
    loss.backward()
    assert torch.equal(loss.detach().reshape(1), vals) and torch.equal(m._flat.grad, grads)
    assert torch.equal(m.logged["loss"], loss.detach())
    loss = m.training_step((x, None), 0)
    m._flat.zero_grad()
    loss.backward()
    assert bool(torch.isfinite(m._flat.grad).all()) and bool(torch.isfinite(loss))


@pytest.mark.parametrize("noise_type", ["gaussian", "masking"])
def test_whole_network_against_float64_at_an_unaligned_width(dev, parity, noise_type):
    """C, S, B = 3, 5, 3: rows of 75 floats - the flattened batch is neither padded nor aligned"""
    C, S, B, seed = 3, 5, 3, 2601
    D = C * S * S
    m = _net(C, S, seed, dev, noise_type=noise_type, noise_level=0.3)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(B, C, S, S, generator=g) * 2 - 1
    if noise_type == "gaussian":
        draw = {"noise": torch.randn(B, C, S, S, generator=g).to(dev)}
        xc = m.corrupt(x.to(dev), **draw)
        assert torch.equal(xc.cpu(), x + draw["noise"].cpu() * 0.3)
    else:
        draw = {"key": -77}
        xc = m.corrupt(x.to(dev), **draw)
        assert np.array_equal(xc.cpu().numpy().reshape(B, D), DR.corrupt_mask(x.numpy().reshape(B, D), -77, "masking", 0.3))
    P64 = {k: v.double() for k, v in DR.dae_init(C, S, seed).items()}
    o, tape = DR.forward(P64, x.double(), xc.cpu().double())
    assert DR.kink_margin(tape) >= 1e-5, "no ReLU input of this case sits at the kink"
    G = DR.backward(P64, tape)
    # the corrupted rows as an unpadded view of an image batch (pitch 75) and as the kernel's own padded output
    for rows, xrows in (("pitch 75", xc.reshape(B, D)), ("pitch 76", m._corrupt_hip(x.to(dev).view(B, D), **draw))):
        (vals, xh), t = m.run(x.to(dev), xrows, True)
        m._flat.zero_grad()
        m.backward_hip(t, torch.ones(1, device=dev))
        parity(f"{noise_type} D75 {rows}: x_hat", rel(xh[:, :D], o["x_hat"]), RTOL)
        parity(f"{noise_type} D75 {rows}: loss", rel(vals[0], o["loss"]), RTOL)
        for n, p in m.named_parameters():
            parity(f"{noise_type} D75 {rows}: grad {n}", rel(p.grad, G[n]), RTOL)


# ----------------------------------------------------------------------------------------------------------------------
# replay and capture
# ----------------------------------------------------------------------------------------------------------------------
CS = (3, 5, 3)      # C, S, B of the replay tests: D = 75


def _batches(dev, n):
    C, S, B = CS
    g = torch.Generator().manual_seed(9)
    return [(torch.rand(B, C, S, S, generator=g).mul(2).sub(1).to(dev), torch.zeros(B, dtype=torch.long, device=dev))
            for _ in range(n)]


def _fast_run(dev, noise_type, use_graph, n=4):
    torch.manual_seed(21)
    m = _net(CS[0], CS[1], 2602, dev, noise_type=noise_type, noise_level=0.3, lr=1e-2)
    opt = m.configure_optimizers()
    f = m.make_fast_step(opt, 1, use_graph)
    losses = [f.step((x.clone(), c.clone()), i).detach().clone().reshape(()) for i, (x, c) in enumerate(_batches(dev, n))]
    st = opt._state(m._flat)
    key = m.__dict__.get("mask_key")
    return f, m, losses, (m._flat.data.clone(), st["m"].clone(), st["v"].clone(), torch.cuda.get_rng_state(dev).clone(),
                          None if key is None else key.clone())


@pytest.mark.parametrize("noise_type", ["gaussian", "salt_and_pepper"])
def test_four_replayed_steps_equal_eager_steps_to_the_bit(dev, noise_type):
    from lgm_hip.optim import FusedAdam
    f, m, la, sa = _fast_run(dev, noise_type, True)
    assert f.mode.startswith("hipGraph"), f.mode
    assert isinstance(f.opt, FusedAdam)
    # four eager steps by hand
    torch.manual_seed(21)
    b = _net(CS[0], CS[1], 2602, dev, noise_type=noise_type, noise_level=0.3, lr=1e-2)
    ob = b.configure_optimizers()
    lb = []
    for i, (x, c) in enumerate(_batches(dev, 4)):
        loss = b.training_step((x, c), i)
        loss.backward()
        ob.step()
        ob.zero_grad()
        lb.append(loss.detach().clone().reshape(()))
    st = ob._state(b._flat)
    assert all(torch.equal(p, q) for p, q in zip(la, lb)), (la, lb)
    assert torch.equal(sa[0], b._flat.data) and torch.equal(sa[1], st["m"]) and torch.equal(sa[2], st["v"])
    assert float(la[0]) != float(la[3])
    assert torch.equal(m.logged["loss"].reshape(()), la[3]), "replay refreshes the logged scalar"
    # a run that captures against the same step object without a graph: warm-up and capture advanced nothing
    g, _, lc, sc = _fast_run(dev, noise_type, False)
    assert not g.mode.startswith("hipGraph")
    assert all(torch.equal(p, q) for p, q in zip(la, lc))
    assert all(torch.equal(p, q) for p, q in zip(sa[:4], sc[:4])), "parameters, Adam moments and the generator state"
    if noise_type == "salt_and_pepper":
        assert sa[4] is not None and torch.equal(sa[4], sc[4]), "the Philox key of the last step"
        assert int(sa[4]) != 0


# ----------------------------------------------------------------------------------------------------------------------
# no-tape paths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_no_tape_paths_give_the_training_forward_bits(fx, dev, case):
    m = _fx_net(fx, case, dev)
    C, S, B = fx[f"{case}:dims"].tolist()
    D = C * S * S
    x = torch.from_numpy(fx[f"{case}:x"]).to(dev)
    xc = torch.from_numpy(fx[f"{case}:corrupted"]).to(dev)
    (vals, xh), tape = m.run(x, xc.reshape(B, D), True)
    img = xh[:, :D].reshape(B, C, S, S)
    m.eval()
    h = m.encode(xc)
    assert tuple(h.shape) == (B, 128) and torch.equal(h, tape[1][2][:, :128])
    assert torch.equal(m.decode(h), img) and tuple(img.shape) == (B, C, S, S)
    assert torch.equal(m.denoise(xc), img) and torch.equal(m(xc), img)
    v = m.validation_step((x, None), 0, corrupted=xc)
    assert torch.equal(v.reshape(1), vals) and torch.equal(m.logged["val_loss"], v) and not v.requires_grad
    v2 = m.validation_step((x, None), 0)                    # its own draw
    assert bool(torch.isfinite(v2))
    # corrupt: its own draw follows the device generator; shape errors are ValueErrors
    torch.manual_seed(3)
    a = m.corrupt(x)
    torch.manual_seed(3)
    assert torch.equal(m.corrupt(x), a) and tuple(a.shape) == (B, C, S, S) and not torch.equal(a, x)
    for bad in (torch.zeros(B, D, device=dev), torch.zeros(B, C, S, S + 1, device=dev)):
        with pytest.raises(ValueError):
            m.encode(bad)
        with pytest.raises(ValueError):
            m.corrupt(bad)
    with pytest.raises(ValueError):
        m.decode(torch.zeros(B, 127, device=dev))
    with pytest.raises(ValueError):
        m.corrupt(x, **({"key": 1} if case == "a" else {"noise": torch.zeros_like(x)}))


def test_linear_refuses_an_activation_without_a_kernel(dev):
    from lgm_hip.nn import Linear
    m = _net(1, 8, 5, dev)
    lin = m.encoder.model[0]
    assert isinstance(lin, Linear)
    x = torch.zeros(2, 64, device=dev)
    for route in ("dense", "generic"):
        lin.fwd_route = route
        with pytest.raises(ValueError, match=route):
            lin.fwd(x, 1)                                   # SiLU: neither route has it for a dense layer


# ----------------------------------------------------------------------------------------------------------------------
# train.py
# ----------------------------------------------------------------------------------------------------------------------
def test_train_entry_runs_the_dae_on_graph_replay(dev, tmp_path):
    """train.py's main() on configs/autoencoder/dae.json at a reduced size: a few graph-replayed steps; last.ckpt loads into a
    CPU DAE whose one CPU step matches the float64 restatement"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "autoencoder", "dae.json")))
    cfg["dataset"].update(img_size=8, batch_size=8)
    cfg["model"]["args"].update(img_size=8)
    path = tmp_path / "dae_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_dae"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('STEPS', m.global_step, m.trainer.fast.mode); print('TRAIN_LOSS', float(m.logged['loss'])); "
            "o = m._optimizers[0]; print('OPT', type(getattr(o, '_opt', o)).__name__)")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "4", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "TRAIN_LOSS", "OPT"))}
    assert lines["STEPS"].startswith("STEPS 4 hipGraph replay"), lines
    assert lines["OPT"] == "OPT FusedAdam", lines
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    sd = torch.load(os.path.join(pkg, "experiments", "DAE", exp, "last.ckpt"), map_location="cpu", weights_only=False)
    assert sd["global_step"] == 4 and list(sd["state_dict"].keys()) == DR.KEYS
    from models.generative.autoencoder.dae import DAE
    cpu = DAE(1, 8)
    cpu.load_state_dict(sd["state_dict"])
    x = torch.rand(8, 1, 8, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1
    torch.manual_seed(2)
    loss = cpu.training_step((x, None), 0)
    torch.manual_seed(2)
    xc = x + torch.randn_like(x) * 0.1
    P = {k: v.double() for k, v in sd["state_dict"].items()}
    want = DR.forward(P, x.double(), xc.double())[0]["loss"]
    assert abs(float(loss.detach()) - float(want)) / abs(float(want)) < 1e-5
