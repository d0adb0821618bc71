"""The MLP VAE on the GPU (csrc/dense.hip, models/generative/vae/vae.py).

Dense kernels (lgm_dense_fwd / lgm_dense_bwd): per element against float64 in units of 2^-24 S under
``oracle.bounds.tolerance(n)``, n = K forward, N for the input gradient, B for the weight and bias gradients, on
``vae_ref.DENSE_SHAPES`` with the operands of ``oracle.bounds.Problem`` (bias on, beta = 1 on a previous gw / gb), all three
activations.  tests/test_vae_host.py shows that the reference's own float32 stays under C_REF_WORST on these shapes.  NaN sits
in every pad lane and padding row of the weights, of their transposed copy and of the bias, and in the pad lanes of the
inputs; NaN guard lanes surround every output and must stay NaN; pad lanes of outputs must be exactly 0.  Equal bits on a
second run, from the scalar-load form of an unaligned input, and at CU margins 0 and 16.

Heads and loss against float64 under (k + 2) u M, u = 2^-24, as tests/test_hip_pixelcnn.py bounds its elementwise kernels:
M is the sum of the absolute values that enter an element, k the roundings on the way.  A device function
counts by its documented worst error in units of u (tanhf 2 ULP = 4, expf 1 ULP = 2), a correctly rounded operation as 1.
  mu, log_var     K / 64 = 2 fmaf per lane, the wave tree 6, the bias 1: k = 9, M = sum |h||w| + |b|.
  z               from the kernel's own mu, log_var: expf 2, product 1, sum 1 (the halving is exact): k = 4.
  kld_part        per term ((1 + v) - m^2) - e^v: 1 + 1 + 1 + 2 + 1 = 6 on M_j = 1 + |v| + m^2 + e^v, then L - 1 additions:
                  k = 6 + L, M = sum_j M_j.
  gmu = gz + c mu, c = kld_weight gloss / (B L): c 2, product 1, sum 1: k = 4.   glv = ((gz eps) 0.5) e^(v/2) + (c 0.5)(e^v - 1):
                  4 on the first term, 6 on the second (c 2, expf 2, the difference 1 - M carries e^v + 1 -, product 1), sum 1:
                  k = 7, M = |gz eps 0.5 e^(v/2)| + |c| 0.5 (e^v + 1).  k_e = 7 for both.
  gb              k_e + ceil(B / 16) + 15 (sixteen row groups) + 1 (beta).   gw   k_e + B (one fmaf per row) + 1 (beta).
  gh              k_e + 2 L (one fmaf chain over both heads).
  x_hat           tanhf: k = 4.   row_part, from the kernel's own x_hat: the difference 1, ceil(D / 256) additions per thread,
                  the wave tree 6, four waves 4: k = 11 + ceil(D / 256), M = sum |x_hat - x|.
  gpre            c = gloss / (B D) 1, x_hat^2 1, the difference 1 (M carries 1 + x_hat^2), product 1: k = 4; exactly 0 where
                  x_hat == x.
  recon, kld      from the kernel's own partials: ceil(B / 64) additions per lane, the tree 6, the quotient 1.  loss: k = 2.

The whole network against tests/golden/vae.npz (tools/make_golden_vae.py) at the project's 1e-4, the graph-replayed step
against eager launches to the bit, the no-tape paths, and train.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vae_ref as VR
from oracle import bounds

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24
NAN = float("nan")
SL = float(np.float32(0.2))                      # the slope as the kernels receive it
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 4, 5
ACTS = ((ACT_NONE, "none"), (ACT_LRELU, "lrelu"), (ACT_TANH, "tanh"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "vae.npz")))


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


def _act64(v, act):
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * SL)
    return torch.tanh(v) if act == ACT_TANH else v


def _dact64(y, act):
    if act == ACT_LRELU:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SL))
    return 1 - y * y if act == ACT_TANH else torch.ones_like(y)


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
# dense kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VR.DENSE_SHAPES, ids=_ids)
def test_dense_forward_per_element(dev, parity, shape):
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

    def run(xin, act):
        yv, ybuf = _guarded(dev, B, Np)
        ops.dense_fwd(xin, wd.data_ptr(), bd.data_ptr(), K, N, yv, act, SL)
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, Np), "guard lanes written"
        return yv.clone()

    for act, name in ACTS:
        y = run(xv, act)
        parity(f"dense_fwd {_ids(shape)} {name} [units of 2^-24 S]", bounds.forward_error_units(y[:, :N], _act64(pre, act), S),
               bounds.tolerance(K))
        assert bool((y[:, N:] == 0).all()), "pad lanes of the output are exactly 0"
        assert torch.equal(run(xv, act), y), "a second run gives the same bits"
        assert torch.equal(run(xo, act), y), "the scalar-load form of the input gives the same bits"
    m0, m16 = _margins(L, lambda: run(xv, ACT_LRELU))
    assert torch.equal(m0, m16), "CU margins 0 and 16 give the same bits"


@pytest.mark.parametrize("shape", VR.DENSE_SHAPES, ids=_ids)
def test_dense_backward_per_element(dev, parity, shape):
    ops = _ops()
    L = ops.lib()
    B, K, N = shape
    t = bounds.Problem("wgrad", (B, 1, 1, K, N, 1, 1, 0)).t
    x, w, gy = t["x"].view(B, K), t["w"].view(N, K), t["gy"].view(B, N)
    gw0, gb0 = t["gw0"].view(N, K), t["gb0"]
    need_gx = shape != (33, 784, 512)                     # the config's first layer has no input gradient
    y0 = torch.randn(B, N, generator=torch.Generator().manual_seed(B + K + N))
    y0 = torch.where(y0 >= 0, 1.0, -1.0) * (y0.abs().clamp(max=1.0) + 1e-3)      # >= 1e-3 from the kink
    Np, Kp = _r4(N), _r4(K)
    wt = _phys(w.T.contiguous(), dev)                     # [Kp][Np], NaN in its pad lanes and padding rows
    xv, _ = _input(x, dev)
    gyv, _ = _input(gy, dev)

    def run(act, yv):
        gwv, gwbuf = _flat_guarded(dev, Np * Kp)
        gbv, gbbuf = _flat_guarded(dev, Np)
        gwv.zero_(), gbv.zero_()
        gwv.view(Np, Kp)[:N, :K] = gw0.to(dev)
        gbv[:N] = gb0.to(dev)
        gxv, gxbuf = _guarded(dev, B, Kp) if need_gx else (None, None)
        ops.dense_bwd(gyv, yv, xv, wt.data_ptr() if need_gx else None, K, N, gxv, gwv.data_ptr(), gbv.data_ptr(), 1.0, act, SL)
        torch.cuda.synchronize()
        assert _flat_guards_intact(gwbuf) and _flat_guards_intact(gbbuf), "guard lanes written"
        assert gxbuf is None or _guards_intact(gxbuf, Kp), "guard lanes written"
        return (gxv.clone() if need_gx else None), gwv.view(Np, Kp).clone(), gbv.clone()

    for act, name in ACTS:
        y = torch.tanh(y0) if act == ACT_TANH else y0
        assert float(y.abs().min()) >= 7e-4
        yv, _ = _input(y, dev)
        g64 = gy.double() * _dact64(y.double(), act)
        gx, gw, gb = run(act, yv)
        if need_gx:
            parity(f"dense_bwd gx {_ids(shape)} {name} [units of 2^-24 S]",
                   bounds.forward_error_units(gx[:, :K], g64 @ w.double(), g64.abs() @ w.abs().double()), bounds.tolerance(N))
            assert bool((gx[:, K:] == 0).all()), "pad lanes of gx are exactly 0"
        ref = torch.cat([(gw0.double() + g64.T @ x.double()).reshape(-1), gb0.double() + g64.sum(0)])
        S = torch.cat([(gw0.abs().double() + g64.abs().T @ x.abs().double()).reshape(-1), gb0.abs().double() + g64.abs().sum(0)])
        got = torch.cat([gw[:N, :K].reshape(-1), gb[:N]])
        parity(f"dense_bwd gw, gb {_ids(shape)} {name} [units of 2^-24 S]", bounds.forward_error_units(got, ref, S),
               bounds.tolerance(B))
        assert bool((gw[N:] == 0).all()) and bool((gw[:, K:] == 0).all()) and bool((gb[N:] == 0).all()), "pads stay exactly 0"
        again = run(act, yv)
        assert all(a is None or torch.equal(a, b_) for a, b_ in zip(again, (gx, gw, gb))), "a second run gives the same bits"
    yv, _ = _input(y0, dev)
    m0, m16 = _margins(L, lambda: run(ACT_LRELU, yv))
    assert all(a is None or torch.equal(a, b_) for a, b_ in zip(m0, m16)), "CU margins 0 and 16 give the same bits"


def test_dense_backward_at_exact_zeros_of_y_follows_torch(dev):
    """LeakyReLU'(0) = slope, torch's choice: with one row and beta = 0 the bias gradient IS g = gy * act'(y)"""
    ops = _ops()
    K, N = 12, 8
    g = torch.Generator().manual_seed(3)
    pre = torch.randn(1, N, generator=g)
    pre[0, ::3] = 0.0
    pre.requires_grad_(True)
    gy, x = torch.randn(1, N, generator=g), torch.randn(1, K, generator=g)
    y = torch.nn.functional.leaky_relu(pre, 0.2)
    y.backward(gy)
    assert int((y == 0).sum()) == 3
    gw = torch.zeros(N, K, device=dev)
    gb = torch.full((N,), NAN, device=dev)                # beta = 0 overwrites whatever is there
    ops.dense_bwd(gy.to(dev), y.detach().to(dev), x.to(dev), None, K, N, None, gw.data_ptr(), gb.data_ptr(), 0.0, ACT_LRELU, SL)
    assert torch.equal(gb.cpu(), pre.grad[0])
    assert torch.equal(gw.cpu(), pre.grad[0][:, None] * x)          # one product per element: no sum to round


# ----------------------------------------------------------------------------------------------------------------------
# heads and loss
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(1, 3), (3, 4), (33, 20), (3, 20), (33, 3), (1, 4)])
def test_heads_forward_and_backward_against_float64(dev, parity, B, L):
    ops = _ops()
    K, Lp = 128, _r4(L)
    g = torch.Generator().manual_seed(100 * B + L)
    h = torch.randn(B, K, generator=g)
    wmu, bmu = torch.randn(L, K, generator=g) / math.sqrt(K), torch.randn(L, generator=g) * 0.1
    wlv, blv = torch.randn(L, K, generator=g) * 0.02, torch.linspace(-8, 8, L)
    eps = torch.randn(B, L, generator=g)
    hv, _ = _input(h, dev)
    wmu_d, wlv_d, bmu_d, blv_d = _phys(wmu, dev), _phys(wlv, dev), _vec(bmu, dev), _vec(blv, dev)
    eps_d = eps.to(dev)
    mu, lv, z, part = ops.vae_head_fwd(hv, K, L, wmu_d.data_ptr(), bmu_d.data_ptr(), wlv_d.data_ptr(), blv_d.data_ptr(), eps_d)
    torch.cuda.synchronize()
    tag = f"B{B} L{L}"
    h64 = h.double()
    for name, got, w_, b_ in (("mu", mu, wmu, bmu), ("log_var", lv, wlv, blv)):
        _within(got[:, :L], h64 @ w_.double().T + b_.double(), h64.abs() @ w_.abs().double().T + b_.abs().double(), 9,
                f"{name} {tag}", parity)
        assert bool((got[:, L:] == 0).all())
    m, v, e = mu[:, :L].double().cpu(), lv[:, :L].double().cpu(), eps.double()
    assert float(v.min()) < -7 and float(v.max()) > 7, "log_var spans [-8, 8]"
    _within(z[:, :L], m + e * torch.exp(v / 2), m.abs() + (e * torch.exp(v / 2)).abs(), 4, f"z {tag}", parity)
    assert bool((z[:, L:] == 0).all())
    _within(part, (1 + v - m * m - v.exp()).sum(1), (1 + v.abs() + m * m + v.exp()).sum(1), 6 + L, f"kld_part {tag}", parity)
    again = ops.vae_head_fwd(hv, K, L, wmu_d.data_ptr(), bmu_d.data_ptr(), wlv_d.data_ptr(), blv_d.data_ptr(), eps_d)
    assert all(torch.equal(a, b_) for a, b_ in zip(again, (mu, lv, z, part)))

    # backward, from the kernel's own mu and log_var
    kw = float(np.float32(0.3))
    gloss = torch.tensor([0.7])
    gz = torch.zeros(B, Lp)
    gz[:, :L] = torch.randn(B, L, generator=g)
    gw0 = [torch.randn(L, K, generator=g) for _ in range(2)]
    gb0 = [torch.randn(L, generator=g) for _ in range(2)]

    def run():
        gw = [_phys(a, dev, 0.0) for a in gw0]
        gb = [_vec(a, dev, 0.0) for a in gb0]
        ghv, ghbuf = _guarded(dev, B, K)
        ops.vae_head_bwd(gz.to(dev), mu, lv, eps_d, gloss.to(dev), kw, hv, K, L, wmu_d.data_ptr(), wlv_d.data_ptr(), ghv,
                         gw[0].data_ptr(), gb[0].data_ptr(), gw[1].data_ptr(), gb[1].data_ptr(), 1.0)
        torch.cuda.synchronize()
        assert _guards_intact(ghbuf, K)
        return ghv.clone(), gw, gb
    gh, gw, gb = run()
    c = kw * float(gloss[0]) / (B * L)
    gzl = gz[:, :L].double()
    G = [gzl + c * m, gzl * e * 0.5 * torch.exp(v / 2) + c * 0.5 * (v.exp() - 1)]
    M = [gzl.abs() + (c * m).abs(), (gzl * e * 0.5 * torch.exp(v / 2)).abs() + abs(c) * 0.5 * (v.exp() + 1)]
    ke = 7
    W = [wmu.double(), wlv.double()]
    _within(gh, G[0] @ W[0] + G[1] @ W[1], M[0] @ W[0].abs() + M[1] @ W[1].abs(), ke + 2 * L, f"gh {tag}", parity)
    for i, name in enumerate(("mu", "log_var")):
        _within(gb[i][:L], gb0[i].double() + G[i].sum(0), gb0[i].abs().double() + M[i].sum(0), ke + (B + 15) // 16 + 16,
                f"gb_{name} {tag}", parity)
        _within(gw[i][:L], gw0[i].double() + G[i].T @ h64, gw0[i].abs().double() + M[i].T @ h64.abs(), ke + B + 1,
                f"gw_{name} {tag}", parity)
        assert bool((gw[i][L:] == 0).all()) and bool((gb[i][L:] == 0).all()), "padding rows stay exactly 0"
    gh2, gw2, gb2 = run()
    assert torch.equal(gh2, gh) and all(torch.equal(a, b_) for a, b_ in zip(gw2 + gb2, gw + gb))


@pytest.mark.parametrize("B,D", [(1, 25), (3, 75), (33, 784), (3, 64)])
def test_tanh_l1_and_the_loss_against_float64(dev, parity, B, D):
    ops = _ops()
    Dp, Lat = _r4(D), 5
    g = torch.Generator().manual_seed(B * 1000 + D)
    pre = torch.randn(B, D, generator=g) * 1.5
    x = torch.rand(B, D, generator=g) * 2 - 1
    prev, _ = _input(pre, dev)
    x_d = x.to(dev).contiguous()                           # rows of D floats: not 16-byte aligned for D = 25, 75
    tag = f"B{B} D{D}"

    def fwd():
        xhv, xbuf = _guarded(dev, B, Dp)
        row = torch.full((B,), NAN, device=dev)
        ops.tanh_l1_fwd(prev, x_d, D, xhv, row)
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
    assert int((diff == 0).sum()) == int(hit.sum())
    _within(row, diff.abs().sum(1), diff.abs().sum(1), 11 + (D + 255) // 256, f"row_part {tag}", parity)
    xh2, row2 = fwd()
    assert torch.equal(xh2[:, :D], xh[:, :D]) and torch.equal(row2, row)

    gloss = torch.tensor([1.3])
    gpv, gbuf = _guarded(dev, B, Dp)
    ops.tanh_l1_bwd(xh, x_d, gloss.to(dev), D, gpv)
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, Dp) and bool((gpv[:, D:] == 0).all())
    c = float(gloss[0]) / (B * D)
    sg = torch.sign(diff)
    _within(gpv[:, :D], sg * c * (1 - xh64 ** 2), sg.abs() * c * (1 + xh64 ** 2), 4, f"gpre {tag}", parity)
    assert bool((gpv[:, :D][hit.to(dev)] == 0).all()), "sign(0) = 0"

    kw = float(np.float32(0.01))
    kpart = (torch.randn(B, generator=g) * 3).to(dev)
    vals = torch.full((3,), NAN, device=dev)
    ops.vae_loss(row, kpart, D, Lat, kw, vals)
    r64, k64 = row.double().cpu(), kpart.double().cpu()
    ks = (B + 63) // 64 + 7
    _within(vals[1], r64.sum() / (B * D), r64.abs().sum() / (B * D), ks, f"recon {tag}", parity)
    _within(vals[2], -0.5 * k64.sum() / (B * Lat), 0.5 * k64.abs().sum() / (B * Lat), ks, f"kld {tag}", parity)
    rc, kl = float(vals[1]), float(vals[2])
    _within(vals[0], rc + kw * kl, abs(rc) + abs(kw * kl), 2, f"loss {tag}", parity)


# ----------------------------------------------------------------------------------------------------------------------
# the whole network
# ----------------------------------------------------------------------------------------------------------------------
def _net(fx, case, dev, **kw):
    from models.generative.vae.vae import VAE
    C, S, L, B = fx[f"{case}:dims"].tolist()
    m = VAE(C, S, latent_dim=L, kld_weight=float(fx["kld_weight"]), **kw)
    m.load_state_dict(VR.vae_init(C, S, L, int(fx[f"{case}:seed"])))
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("route", ["dense", "generic", "generic_bwd"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_whole_network_against_the_reference_fixture(fx, dev, parity, monkeypatch, case, route):
    """every route of ``lgm_hip.nn.Linear``: the dense kernels, the generic 1x1 kernels in both directions (where the
    operands allow: case b's image rows of 75 floats stay on the dense kernels), and the generic backward alone"""
    from lgm_hip.nn import Linear
    monkeypatch.setattr(Linear, "fwd_route", "generic" if route == "generic" else "dense")
    monkeypatch.setattr(Linear, "bwd_route", "dense" if route == "dense" else "generic")
    m = _net(fx, case, dev)
    C, S, L, B = fx[f"{case}:dims"].tolist()
    x, eps = torch.from_numpy(fx[f"{case}:x"]).to(dev), torch.from_numpy(fx[f"{case}:eps"]).to(dev)
    (vals, xh, mu, lv), tape = m.run(x, eps, True)
    m._flat.zero_grad()
    m.backward_hip(tape, torch.ones(1, device=dev))
    torch.cuda.synchronize()
    parity(f"case {case} {route}: mu", rel(mu[:, :L], fx[f"{case}:mu"]), RTOL)
    parity(f"case {case} {route}: log_var", rel(lv[:, :L], fx[f"{case}:log_var"]), RTOL)
    parity(f"case {case} {route}: x_hat", rel(xh[:, :C * S * S], fx[f"{case}:x_hat"]), RTOL)
    for i, name in enumerate(("loss", "recon", "kld")):
        parity(f"case {case} {route}: {name}", rel(vals[i], fx[f"{case}:{name}"]), RTOL)
    for n, p in m.named_parameters():
        parity(f"case {case} {route}: grad {n}", VR.fixture_grad_error(fx, case, n, p.grad), RTOL)
    # the same through autograd's one Function, eps drawn inside: finite, and the logged scalars are the three losses
    loss = m.training_step((x, None), 0)
    loss.backward()
    assert bool(torch.isfinite(m._flat.grad).all()) and set(m.logged) >= {"train_loss", "train_recon_loss", "train_kld"}
    assert torch.equal(m.logged["train_loss"], loss.detach())
    with torch.no_grad():
        v = m.validation_step((x, None), 0)
    assert bool(torch.isfinite(v)) and "val_kld" in m.logged


def _batches(fx, case, dev, n):
    C, S, L, B = fx[f"{case}:dims"].tolist()
    g = torch.Generator().manual_seed(9)
    return [(torch.rand(B, C, S, S, generator=g).mul(2).sub(1).to(dev), torch.zeros(B, dtype=torch.long, device=dev))
            for _ in range(n)]


def _fast_run(fx, dev, use_graph, accumulate, clip, n):
    torch.manual_seed(21)
    m = _net(fx, "b", dev, lr=1e-2)
    opt = m.configure_optimizers()
    if clip:
        opt.max_grad_norm = 0.05
    f = m.make_fast_step(opt, 1, use_graph, accumulate)
    losses = [f.step((x.clone(), c.clone()), i).detach().clone().reshape(()) for i, (x, c) in enumerate(_batches(fx, "b", dev, n))]
    st = opt._state(m._flat)
    return f, m, losses, (m._flat.data.clone(), st["m"].clone(), st["v"].clone())


def test_three_fast_steps_equal_eager_launches_to_the_bit(fx, dev):
    from lgm_hip.optim import FusedAdam
    for clip in (False, True):
        f, m, la, sa = _fast_run(fx, dev, True, 1, clip, 3)
        assert f.mode.startswith("hipGraph"), f.mode
        assert isinstance(f.opt, FusedAdam)
        torch.manual_seed(21)
        b = _net(fx, "b", dev, lr=1e-2)
        ob = b.configure_optimizers()
        if clip:
            ob.max_grad_norm = 0.05
        lb = []
        for i, (x, c) in enumerate(_batches(fx, "b", dev, 3)):
            loss = b.training_step((x, c), i)
            loss.backward()
            ob.step()
            ob.zero_grad()
            lb.append(loss.detach().clone().reshape(()))
        st = ob._state(b._flat)
        assert all(torch.equal(p, q) for p, q in zip(la, lb)), (clip, la, lb)
        assert torch.equal(sa[0], b._flat.data) and torch.equal(sa[1], st["m"]) and torch.equal(sa[2], st["v"]), clip
        assert float(la[0]) != float(la[2])
        assert torch.equal(m.logged["train_loss"].reshape(()), la[2]), "replay refreshes the logged scalars"
    # two micro-batches per optimizer step: the replayed step against the same step object issuing eager launches
    f, _, la, sa = _fast_run(fx, dev, True, 2, False, 4)
    assert f.mode.startswith("hipGraph"), f.mode
    g, _, lb, sb = _fast_run(fx, dev, False, 2, False, 4)
    assert not g.mode.startswith("hipGraph")
    assert all(torch.equal(p, q) for p, q in zip(la, lb)) and all(torch.equal(p, q) for p, q in zip(sa, sb))


def test_no_tape_paths_against_float64_and_the_draw(fx, dev, parity):
    m = _net(fx, "a", dev)
    m.eval()
    C, S, L, B = fx["a:dims"].tolist()
    P = {k: v.double() for k, v in VR.vae_init(C, S, L, int(fx["a:seed"])).items()}
    x = torch.from_numpy(fx["a:x"])
    mu64, lv64, _, _ = VR.encode(P, x.double())
    mu, lv = m.encode(x.to(dev))
    assert tuple(mu.shape) == (B, L)
    parity("encode: mu", rel(mu, mu64), RTOL)
    parity("encode: log_var", rel(lv, lv64), RTOL)
    z = torch.randn(5, L, generator=torch.Generator().manual_seed(4))
    img = m.decode(z.to(dev))
    assert tuple(img.shape) == (5, C, S, S)
    parity("decode", rel(img, VR.decode(P, z.double())[0]), RTOL)
    assert torch.equal(m.sample(5, z=z.to(dev)), img)
    parity("reconstruct", rel(m.reconstruct(x.to(dev)), VR.decode(P, mu64)[0]), RTOL)
    xh, mu_f, _ = m(x.to(dev))
    assert tuple(xh.shape) == (B, C, S, S) and torch.equal(mu_f, mu)
    torch.manual_seed(3)
    a = m.sample(5)
    torch.manual_seed(3)
    assert torch.equal(m.sample(5), a) and tuple(a.shape) == (5, C, S, S) and float(a.abs().max()) <= 1.0
    with pytest.raises(ValueError):
        m.decode(torch.zeros(3, L + 1, device=dev))


def test_train_entry_runs_the_vae_on_graph_replay(dev, tmp_path):
    """train.py's main() on configs/vae/vae.json at a reduced size: a few graph-replayed steps; last.ckpt loads into a CPU
    VAE whose one CPU step matches the float64 restatement"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "vae", "vae.json")))
    cfg["dataset"].update(img_size=8, batch_size=8)
    cfg["model"]["args"].update(img_size=8, latent_dim=4)
    path = tmp_path / "vae_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_vae"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('STEPS', m.global_step, m.trainer.fast.mode); print('TRAIN_LOSS', float(m.logged['train_loss'])); "
            "o = m._optimizers[0]; print('OPT', type(getattr(o, '_opt', o)).__name__)")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "4", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "TRAIN_LOSS", "OPT"))}
    assert lines["STEPS"].startswith("STEPS 4 hipGraph replay"), lines
    assert lines["OPT"] == "OPT FusedAdam", lines
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    sd = torch.load(os.path.join(pkg, "experiments", "VAE", exp, "last.ckpt"), map_location="cpu", weights_only=False)
    assert sd["global_step"] == 4 and list(sd["state_dict"].keys()) == VR.KEYS
    from models.generative.vae.vae import VAE
    cpu = VAE(1, 8, latent_dim=4)
    cpu.load_state_dict(sd["state_dict"])
    x = torch.rand(8, 1, 8, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1
    torch.manual_seed(2)
    loss = cpu.training_step((x, None), 0)
    torch.manual_seed(2)
    eps = torch.randn(8, 4)
    P = {k: v.double() for k, v in sd["state_dict"].items()}
    want = VR.forward(P, x.double(), eps.double(), 1e-2)[0]["loss"]
    assert abs(float(loss.detach()) - float(want)) / abs(float(want)) < 1e-5
