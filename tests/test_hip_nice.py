"""The NICE flow on the GPU (csrc/nice.hip, models/generative/flow/nice.py).

lgm_nice_couple: one correctly rounded operation - equal bits with the CPU's float32 x + t / x - t on the slice, x's bits
elsewhere; in place and out of place; NaN in every pad lane of the inputs and in the rows around them; pad lanes of the output
+0; the NaN frame around the output untouched; the 16-byte and the scalar form to the bit.

Scaling layer and loss against float64 under (k + 2) u M, u = 2^-24, as tests/test_hip_dae.py bounds its elementwise kernels:
M is the sum of the absolute values that enter an element, k the roundings on the way.  expf counts by its
documented worst error of 1 ULP = 2 u, a correctly rounded operation as 1.
  z               expf 2, the product 1: k = 3, M = |h| e^(+-s).
  row_part        from the kernel's own z: the square 1; a thread adds the 4 elements of a quad and ceil(D / 1024) quads:
                  4 ceil(D / 1024) additions, the wave tree 6, four waves 4: k = 11 + 4 ceil(D / 1024), M = sum z^2.
  mean_ll         from the kernel's own partials: ceil(B / 64) additions per lane, the tree 6, the quotient 1, the constant
                  fl(0.5 D log 2 pi) 1, the difference 1: k = ceil(B / 64) + 9, M = 0.5 sum_b row_part / B + 0.5 D log 2 pi.
  sum log_scale   ceil(D / 64) additions per lane, the tree 6: k = ceil(D / 64) + 6, M = sum |log_scale|.
  loss            one more operation on the two: k = max of the two + 1, M = the sum of theirs.
  gh              c = gloss / B 1, c z 1, expf 2, the product 1: k = 5, M = |c z| e^s.
  gls             per term c 1, c z 1, (c z) z 1; B additions; + -gloss 1; beta gls 1, the last sum 1: k = B + 6,
                  M = |beta gls| + sum_b |c| z^2 + |gloss|.

row_part, mean_ll, the sum and the loss are bounded against float64 sums of what the kernel itself read (its own float32 z,
its own partials): each link of the chain z -> row_part -> loss is held to float64, not the chain end to end.

The whole network against tests/golden/nice.npz (tools/make_golden_nice.py) at the project's 1e-4 under the four route
settings of ``lgm_hip.nn.Linear`` - with halves of 10 and 3 lanes every lane slice stays on the dense kernels, so only the
second Linear's forward changes there - and, with halves of 4 and 12 lanes, against the float64 restatement on all four routes
with call counters that show the generic kernels taking the slices, forward and backward; the float64 restatement with
``alternate`` and ``exact_logdet``, the round trip on the device, the no-tape paths, the graph-replayed step against eager
launches and against plain training_step / backward / opt.step to the bit (also two micro-batches per step), and train.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nice_ref as NR

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24
NAN = float("nan")
K_SCALE = 3
# (B, D, off, n, pitch of x): the last is the config's layer at B = 32
COUPLE_SHAPES = [(1, 2, 1, 1, 2), (3, 6, 3, 3, 6), (5, 20, 10, 10, 20), (5, 20, 0, 10, 20), (7, 10, 5, 5, 13), (32, 784, 392, 392, 784)]
SCALE_D = (2, 6, 20, 784)
SCALE_B = (1, 5, 64, 130)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "nice.npz")))


def _ops():
    from lgm_hip import ops
    return ops


def _r4(n):
    return (n + 3) // 4 * 4


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a.reshape(-1) - b.reshape(-1)).norm() / b.norm().clamp_min(1e-30))


def _last_kernel():
    return _ops().lib()._dll.lgm_last_kernel().decode()


def _framed(dev, B, W, pitch, shift=0, values=None):
    """A [B, W] view with row pitch ``pitch`` inside a NaN-filled buffer: one guard row before and after, NaN in lanes
    [W, pitch) of every row; ``shift`` floats off a 16-byte boundary.  -> (the view, the buffer)"""
    assert pitch >= W
    buf = torch.full(((B + 2) * pitch + 8,), NAN, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + (B + 2) * pitch].view(B + 2, pitch)[1:B + 1, :W]
    if values is not None:
        v.copy_(values.to(dev))
    return v, buf


def _frame_intact(buf, view, live):
    """every float of ``buf`` outside the first ``live`` lanes of the view's rows is still NaN"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    start = (view.data_ptr() - buf.data_ptr()) // 4
    for b in range(view.shape[0]):
        mask[start + b * view.stride(0):start + b * view.stride(0) + live] = False
    return bool(torch.isnan(buf[mask]).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


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


# ----------------------------------------------------------------------------------------------------------------------
# the coupling
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", COUPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_couple_equals_the_cpu_float32_result_to_the_bit(dev, shape):
    ops = _ops()
    L = ops.lib()
    B, D, off, n, xp = shape
    Dp = _r4(D)
    g = torch.Generator().manual_seed(31 * B + D + off)
    x = torch.rand(B, D, generator=g) * 2 - 1
    t = torch.randn(B, n, generator=g)
    x[0, 0 if off else D - 1] = -0.0                                      # a sign bit survives outside the slice
    for sign in (1, -1):
        want = x.clone()
        want[:, off:off + n] = x[:, off:off + n] + t if sign > 0 else x[:, off:off + n] - t
        for form, shift in (("aligned", 0), ("4 bytes off", 1)):
            for in_place in (False, True):
                xpitch = max(xp, Dp) if in_place and xp < Dp else xp      # in place x is an output too: its pitch holds r4(D)
                xv, xbuf = _framed(dev, B, D, xpitch, shift, x)
                tv, _ = _framed(dev, B, n, _r4(n) + 4, shift, t)
                if in_place:
                    ov, obuf = xbuf[(xv.data_ptr() - xbuf.data_ptr()) // 4:].as_strided((B, Dp), (xpitch, 1)), xbuf
                    assert ov.data_ptr() == xv.data_ptr()
                else:
                    ov, obuf = _framed(dev, B, Dp, Dp + 4, shift)
                ops.nice_couple(xv, tv, off, sign, ov)
                torch.cuda.synchronize()
                kern = _last_kernel()
                vec = shift == 0 and off % 4 == 0 and xpitch % 4 == 0
                assert kern == f"nice_couple_kernel<{'true' if vec else 'false'}>", (kern, form, in_place)
                assert _frame_intact(obuf, ov, Dp), ("sentinel rows and lanes around out", form, in_place)
                assert torch.equal(_bits(ov[:, :D]), _bits(want)), (sign, form, in_place)
                assert torch.equal(_bits(ov[:, D:]), torch.zeros(B, Dp - D, dtype=torch.int32)), "pad lanes are +0"
        # determinism: a second run and both CU margins
        xv, _ = _framed(dev, B, D, xp, 0, x)
        tv, _ = _framed(dev, B, n, _r4(n) + 4, 0, t)

        def run():
            o = torch.full((B, Dp), NAN, device=dev)
            ops.nice_couple(xv, tv, off, sign, o)
            return o
        first = run()
        assert torch.equal(_bits(run()), _bits(first))
        m0, m16 = _margins(L, run)
        assert torch.equal(_bits(m0), _bits(first)) and torch.equal(_bits(m16), _bits(first))
    if shape == COUPLE_SHAPES[-1]:
        assert xp % 4 == 0 and off % 4 == 0, "the config's layer runs the 16-byte form"


def test_couple_undoes_itself_only_up_to_two_roundings(dev):
    """(x + t) - t is not x: the inverse costs two roundings per layer, which the round-trip bound counts"""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x, t = torch.rand(8, 12, generator=g), torch.randn(8, 4, generator=g) * 100
    s = ops.nice_couple(x.to(dev), t.to(dev), 4, 1, torch.empty(8, 12, device=dev))
    ops.nice_couple(s, t.to(dev), 4, -1, s)
    assert torch.equal(s.cpu()[:, 4:8], (x[:, 4:8] + t) - t) and torch.equal(_bits(s.cpu()[:, :4]), _bits(x[:, :4]))
    assert float((s.cpu() - x).abs().max()) <= 2 * U * 2 * float(t.abs().max() + 1)


# ----------------------------------------------------------------------------------------------------------------------
# scaling layer, loss, backward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SCALE_B)
@pytest.mark.parametrize("D", SCALE_D)
def test_scaling_layer_loss_and_backward_against_float64(dev, parity, D, B):
    ops = _ops()
    L = ops.lib()
    Dp = _r4(D)
    g = torch.Generator().manual_seed(B * 1000 + D)
    h = torch.randn(B, D, generator=g) * 1.5
    ls = torch.rand(D, generator=g) * 4 - 2                     # log_scale in +-2
    ls[0], ls[D - 1] = 2.0, -2.0
    tag = f"B{B} D{D}"
    ls_a = torch.full((Dp + 4,), NAN, device=dev)                # 16-byte aligned, NaN after its D values
    ls_a[:D] = ls.to(dev)
    ls_o = torch.full((D + 5,), NAN, device=dev)[1:]             # 4 bytes off
    ls_o[:D] = ls.to(dev)
    forms = (("aligned", 0, ls_a), ("4 bytes off", 1, ls_o))

    def fwd(shift, lsd, reverse, hin=h, with_rows=True):
        hv, _ = _framed(dev, B, D, Dp + 4, shift, hin)
        zv, zbuf = _framed(dev, B, Dp, Dp + 4, shift)
        row, rbuf = _framed(dev, 1, B, B, 0)
        ops.nice_scale_fwd(hv, lsd.data_ptr(), D, reverse, zv, row[0] if with_rows else None)
        torch.cuda.synchronize()
        vec = shift == 0
        assert _last_kernel() == f"nice_scale_fwd_kernel<{'true' if vec else 'false'}>"
        assert _frame_intact(zbuf, zv, Dp) and _frame_intact(rbuf, row, B if with_rows else 0)
        assert torch.equal(_bits(zv[:, D:]), torch.zeros(B, Dp - D, dtype=torch.int32)), "pad lanes are +0"
        return zv[:, :D].clone(), row[0].clone()

    saved = {}
    for reverse in (False, True):
        z, row = fwd(0, ls_a, reverse)
        e64 = torch.exp(-ls.double() if reverse else ls.double())
        _within(z, h.double() * e64, h.double().abs() * e64, K_SCALE, f"z {tag} reverse={reverse}", parity)
        z64 = z.double().cpu()
        sq = (z64 ** 2).sum(1)
        _within(row, sq, sq, 11 + 4 * ((D + 1023) // 1024), f"row_part {tag} reverse={reverse}", parity)
        z2, row2 = fwd(0, ls_a, reverse)
        assert torch.equal(z2, z) and torch.equal(row2, row), "a second run gives the same bits"
        z3, row3 = fwd(1, ls_o, reverse)
        assert torch.equal(z3, z) and torch.equal(row3, row), "both load forms give the same bits"
        z4, row4 = fwd(0, ls_a, reverse, with_rows=False)
        assert torch.equal(z4, z) and bool(torch.isnan(row4).all()), "without row_part: the same z, nothing else written"
        (za, ra), (zb, rb) = _margins(L, lambda: fwd(0, ls_a, reverse))
        assert torch.equal(za, z) and torch.equal(zb, z) and torch.equal(ra, row) and torch.equal(rb, row), "CU margins 0 and 16"
        saved[reverse] = (z, row)
    z, row = saved[False]
    z64, r64, ls64 = z.double().cpu(), row.double().cpu(), ls.double()

    # ---- the loss, from the kernel's own partials ------------------------------------------------------------------------
    const = 0.5 * D * NR.LOG_2PI
    ll64, sl64 = -0.5 * r64.sum() / B - const, ls64.sum()
    m_ll, m_sl = 0.5 * r64.sum() / B + const, ls64.abs().sum()
    k_ll, k_sl = (B + 63) // 64 + 9, (D + 63) // 64 + 6
    for exact in (False, True):
        vals, vbuf = _framed(dev, 1, 3, 3, 0)
        for lsd in (ls_a, ls_o):
            vals.fill_(NAN)
            ops.nice_loss(row, lsd.data_ptr(), D, exact, vals[0])
            torch.cuda.synchronize()
            assert _frame_intact(vbuf, vals, 3)
            if lsd is ls_a:
                v = vals[0].clone()
            assert torch.equal(vals[0], v), "the same bits from either log_scale and on a second run"
        _within(v[1], ll64, m_ll, k_ll, f"mean_ll {tag}", parity)
        _within(v[2], sl64, m_sl, k_sl, f"sum log_scale {tag}", parity)
        want = -(ll64 + sl64) if exact else -(ll64 - sl64)
        _within(v[0], want, m_ll + m_sl, max(k_ll, k_sl) + 1, f"loss {tag} exact={exact}", parity)
        assert bool(v[0] == (-(v[1] + v[2]) if exact else -(v[1] - v[2]))), "one float32 operation on the two, then the sign"
        va, vb = _margins(L, lambda: ops.nice_loss(row, ls_a.data_ptr(), D, exact, torch.empty(3, device=dev)).clone())
        assert torch.equal(va, v) and torch.equal(vb, v)

    # ---- the backward, from the kernel's own z ----------------------------------------------------------------------------
    gl = 1.3
    gl_d = torch.tensor([gl], device=dev)
    gl32 = float(torch.tensor(gl, dtype=torch.float32))
    c64 = gl32 / B
    gls0 = torch.randn(D, generator=g)

    def bwd(shift, lsd, exact, beta):
        zv, _ = _framed(dev, B, D, Dp + 4, shift, z)
        gv, gbuf = _framed(dev, B, Dp, Dp + 4, shift)
        gls, lbuf = _framed(dev, 1, D, D, shift)
        if beta:
            gls[0].copy_(gls0.to(dev))                         # beta = 0 overwrites the NaN that is there
        ops.nice_scale_bwd(zv, lsd.data_ptr(), gl_d, D, exact, gv, gls.data_ptr(), beta)
        torch.cuda.synchronize()
        assert _last_kernel() == f"nice_scale_bwd_kernel<{'true' if shift == 0 else 'false'}>"
        assert _frame_intact(gbuf, gv, Dp) and _frame_intact(lbuf, gls, D)
        assert torch.equal(_bits(gv[:, D:]), torch.zeros(B, Dp - D, dtype=torch.int32)), "pad lanes are +0"
        return gv[:, :D].clone(), gls[0].clone()

    for exact in (False, True):
        for beta in (0.0, 1.0):
            gh, gls = bwd(0, ls_a, exact, beta)
            e64 = torch.exp(ls64)
            _within(gh, c64 * z64 * e64, abs(c64) * z64.abs() * e64, 5, f"gh {tag}", parity)
            col = (c64 * z64 * z64).sum(0)
            want = beta * gls0.double() + col + (-gl32 if exact else gl32)
            mag = beta * gls0.double().abs() + col.abs() + abs(gl32)
            _within(gls, want, mag, B + 6, f"gls {tag} exact={exact} beta={beta}", parity)
            gh2, gls2 = bwd(0, ls_a, exact, beta)
            assert torch.equal(gh2, gh) and torch.equal(gls2, gls), "a second run gives the same bits"
            gh3, gls3 = bwd(1, ls_o, exact, beta)
            assert torch.equal(gh3, gh) and torch.equal(gls3, gls), "both load forms give the same bits"
    (ga, la), (gb, lb) = _margins(L, lambda: bwd(0, ls_a, True, 1.0))
    assert torch.equal(ga, gh) and torch.equal(gb, gh) and torch.equal(la, gls) and torch.equal(lb, gls), "CU margins 0 and 16"


# ----------------------------------------------------------------------------------------------------------------------
# the whole network
# ----------------------------------------------------------------------------------------------------------------------
def _net(D, L, H, P, dev, **kw):
    from models.generative.flow.nice import NICE
    m = NICE(D, L, H, **kw)
    m.load_state_dict(P)
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


def _fx_net(fx, case, dev, **kw):
    D, B = fx[f"{case}:dims"].tolist()
    P = NR.nice_init(D, int(fx["layers"]), int(fx["hidden"]), int(fx[f"{case}:seed"]))
    return _net(D, int(fx["layers"]), int(fx["hidden"]), P, dev, **kw), P


def _routes(monkeypatch, fwd_route, bwd_route):
    from lgm_hip.nn import Linear
    monkeypatch.setattr(Linear, "fwd_route", fwd_route)
    monkeypatch.setattr(Linear, "bwd_route", bwd_route)


@pytest.mark.parametrize("bwd_route", ["dense", "generic"])
@pytest.mark.parametrize("fwd_route", ["dense", "generic"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_whole_network_against_the_reference_fixture(fx, dev, parity, monkeypatch, case, fwd_route, bwd_route):
    _routes(monkeypatch, fwd_route, bwd_route)
    m, _ = _fx_net(fx, case, dev)
    D, B = fx[f"{case}:dims"].tolist()
    x = torch.from_numpy(fx[f"{case}:x"]).to(dev)
    tag = f"case {case} {fwd_route}/{bwd_route}"
    (vals, z, _), tape = m.run(x, True)
    m._flat.zero_grad()
    m.backward_hip(tape, torch.ones(1, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(_bits(tape[0][-1][:, :D // 2]), _bits(x[:, :D // 2])), "the reference never transforms the first half"
    parity(f"{tag}: z", rel(z[:, :D], fx[f"{case}:z"]), RTOL)
    parity(f"{tag}: loss", rel(vals[0], fx[f"{case}:loss"]), RTOL)
    for n, p in m.named_parameters():
        parity(f"{tag}: grad {n}", NR.fixture_grad_error(fx, case, n, p.grad), RTOL)
    parity(f"{tag}: inverse", rel(m.inverse(torch.from_numpy(fx[f"{case}:z"]).to(dev)), fx[f"{case}:inverse"]), RTOL)
    grads = m._flat.grad.clone()
    assert bool(torch.isfinite(grads).all()), "pad lanes of the flat gradient included"
    # the same through autograd's one Function: the same bits
    loss = m.training_step((x, None), 0)
    m._flat.zero_grad()
    loss.backward()
    assert torch.equal(loss.detach().reshape(1), vals[:1]) and torch.equal(m._flat.grad, grads)
    assert torch.equal(m.logged["train_loss"], loss.detach())
    assert torch.equal(m(x), z[:, :D]), "forward() is the same launches without a tape"


@pytest.mark.parametrize("dims", [(20, 5), (6, 3)], ids=lambda d: "x".join(map(str, d)))
def test_whole_network_against_float64_with_alternate_and_exact_logdet(dev, parity, dims):
    D, B = dims
    L, H, seed = 4, 24, 2601
    P = NR.nice_init(D, L, H, seed)
    m = _net(D, L, H, P, dev, alternate=True, exact_logdet=True)
    x = torch.rand(B, D, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
    P64 = {k: v.double() for k, v in P.items()}
    o, tape = NR.forward(P64, x.double(), True, True)
    assert NR.kink_margin(tape) >= 1e-5, "no LeakyReLU input of this case sits at the kink"
    G = NR.backward(P64, tape, gloss=0.7)
    (vals, z, _), t = m.run(x.to(dev), True)
    m._flat.zero_grad()
    m.backward_hip(t, torch.full((1,), 0.7, device=dev))
    tag = f"alternate, exact D{D}"
    h = t[0][-1][:, :D]
    assert not bool((h == x.to(dev)).any()), "every lane is transformed"
    parity(f"{tag}: z", rel(z[:, :D], o["z"]), RTOL)
    parity(f"{tag}: loss", rel(vals[0], o["loss"]), RTOL)
    parity(f"{tag}: mean_ll", rel(vals[1], o["mean_ll"]), RTOL)
    parity(f"{tag}: sum log_scale", rel(vals[2], o["sum_ls"]), RTOL)
    for n, p in m.named_parameters():
        parity(f"{tag}: grad {n}", rel(p.grad, G[n]), RTOL)
    parity(f"{tag}: log_prob", rel(m.log_prob(x.to(dev)), o["log_prob"]), RTOL)
    # an image batch is flattened as a view and keeps its shape
    if D == 20:
        mi = _net(D, L, H, P, dev, alternate=True, exact_logdet=True, img_channels=5, img_size=2)
        xi = x.to(dev).reshape(B, 5, 2, 2)
        zi = mi(xi)
        assert tuple(zi.shape) == (B, 5, 2, 2) and torch.equal(zi.reshape(B, D), z[:, :D])
        assert tuple(mi.sample(B, z=z[:, :D].contiguous()).shape) == (B, 5, 2, 2)


def _counted(monkeypatch, names):
    """wrap ``ops.<name>`` for every name -> {name: calls so far}"""
    ops = _ops()
    calls = {n: 0 for n in names}
    for n in names:
        def wrapper(*a, _n=n, _f=getattr(ops, n), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, n, wrapper)
    return calls


@pytest.mark.parametrize("bwd_route", ["dense", "generic"])
@pytest.mark.parametrize("fwd_route", ["dense", "generic"])
@pytest.mark.parametrize("dims", [(8, 5), (24, 3)], ids=lambda d: "x".join(map(str, d)))
def test_whole_network_on_the_four_routes_with_halves_the_generic_kernels_take(dev, parity, monkeypatch, dims, fwd_route, bwd_route):
    """Halves of 4 and of 12 lanes: a multiple of 4, so a lane slice of the state (at lane 0 and at lane D / 2: ``alternate``)
    and of the gradient buffer goes to the generic 1x1 kernels as a pitched map where the route says so - as the config's
    392-lane halves do.  The counters show which kernels ran; z, loss, every gradient and the inverse against float64."""
    D, B = dims
    L, H, seed = 4, 24, 2611
    _routes(monkeypatch, fwd_route, bwd_route)
    calls = _counted(monkeypatch, ("dense_fwd", "conv_xy", "dense_bwd", "conv_bwd_generic"))
    P = NR.nice_init(D, L, H, seed)
    m = _net(D, L, H, P, dev, alternate=True, exact_logdet=True)
    x = torch.rand(B, D, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
    P64 = {k: v.double() for k, v in P.items()}
    o, tape = NR.forward(P64, x.double(), True, True)
    assert NR.kink_margin(tape) >= 1e-5, "no LeakyReLU input of this case sits at the kink"
    G = NR.backward(P64, tape, gloss=0.7)
    (vals, z, _), t = m.run(x.to(dev), True)
    fwd_calls = dict(calls)
    m._flat.zero_grad()
    m.backward_hip(t, torch.full((1,), 0.7, device=dev))
    torch.cuda.synchronize()
    gen_f, gen_b = fwd_route == "generic", bwd_route == "generic"
    assert fwd_calls["dense_fwd"] == (0 if gen_f else 2 * L) and fwd_calls["conv_xy"] == (2 * L if gen_f else 0), fwd_calls
    assert calls["dense_bwd"] == (0 if gen_b else 2 * L) and calls["conv_bwd_generic"] == (2 * L if gen_b else 0), calls
    assert calls["dense_fwd"] == fwd_calls["dense_fwd"], "the backward runs no forward kernel of the dense section"
    tag = f"slices D{D} {fwd_route}/{bwd_route}"
    assert not bool((t[0][-1][:, :D] == x.to(dev)).any()), "every lane is transformed"
    parity(f"{tag}: z", rel(z[:, :D], o["z"]), RTOL)
    parity(f"{tag}: loss", rel(vals[0], o["loss"]), RTOL)
    for n, p in m.named_parameters():
        parity(f"{tag}: grad {n}", rel(p.grad, G[n]), RTOL)
    assert bool(torch.isfinite(m._flat.grad).all()) and bool(torch.isfinite(m._flat.data).all())
    z64 = o["z"].float().to(dev)
    before = dict(calls)
    inv = m.inverse(z64)
    assert calls["conv_xy"] - before["conv_xy"] == (2 * L if gen_f else 0) and \
        calls["dense_fwd"] - before["dense_fwd"] == (0 if gen_f else 2 * L)
    parity(f"{tag}: inverse", rel(inv, NR.inverse(P64, z64.double().cpu(), True)), RTOL)
    # the step through autograd's one Function: the same bits as the launches above
    grads = m._flat.grad.clone()
    loss = m.training_step((x.to(dev), None), 0)
    m._flat.zero_grad()
    (0.7 * loss).backward()
    assert torch.equal(loss.detach().reshape(1), vals[:1]) and torch.equal(m._flat.grad, grads)


@pytest.mark.parametrize("alternate", [False, True])
@pytest.mark.parametrize("dims", [(20, 5, 256), (6, 3, 256), (784, 4, 24)], ids=lambda d: "x".join(map(str, d)))
def test_round_trip_on_the_device(dev, parity, dims, alternate):
    """inverse(forward(x)) within (2 L + 2 k_scale + 2) u M per element, M the largest absolute state value of the float64
    restatement: each layer costs the two roundings of (x + t) - t, the scaling layer k_scale each way"""
    D, B, H = dims
    L = 4
    P = NR.nice_init(D, L, H, 77)
    m = _net(D, L, H, P, dev, alternate=alternate)
    x = torch.rand(B, D, generator=torch.Generator().manual_seed(78)) * 2 - 1
    _, tape = NR.forward({k: v.double() for k, v in P.items()}, x.double(), alternate)
    M = NR.max_state(tape)
    back = m.inverse(m(x.to(dev)))
    err = float((back.double().cpu() - x.double()).abs().max())
    parity(f"round trip D{D} alternate={alternate} [|err| / ((2 L + 2 k_scale + 2) u M)]", err / ((2 * L + 2 * K_SCALE + 2) * U * M), 1.0)
    assert torch.equal(m.inverse(m(x.to(dev))), back)


@pytest.mark.parametrize("case", ["a", "b"])
def test_no_tape_paths(fx, dev, parity, case):
    m, P = _fx_net(fx, case, dev)
    D, B = fx[f"{case}:dims"].tolist()
    x = torch.from_numpy(fx[f"{case}:x"]).to(dev)
    zf = torch.from_numpy(fx[f"{case}:z"]).to(dev)
    (vals, z, _), _ = m.run(x, True)
    m.eval()
    assert torch.equal(m(x), z[:, :D]) and not m(x).requires_grad
    assert torch.equal(x, torch.from_numpy(fx[f"{case}:x"]).to(dev)), "the batch is left alone"
    v = m.validation_step((x, None), 0)
    assert torch.equal(v.reshape(1), vals[:1]) and torch.equal(m.logged["val_loss"], v) and not v.requires_grad
    P64 = {k: v_.double() for k, v_ in P.items()}
    o, _ = NR.forward(P64, x.double().cpu())
    parity(f"case {case}: log_prob", rel(m.log_prob(x), o["log_prob"]), RTOL)
    inv = m.inverse(zf)
    assert torch.equal(zf, torch.from_numpy(fx[f"{case}:z"]).to(dev)), "z is left alone"
    parity(f"case {case}: inverse against the fixture", rel(inv, fx[f"{case}:inverse"]), RTOL)
    parity(f"case {case}: inverse against float64", rel(inv, NR.inverse(P64, zf.double().cpu())), RTOL)
    assert torch.equal(m(zf, reverse=True), inv) and torch.equal(m.sample(B, z=zf), inv) and tuple(inv.shape) == (B, D)
    torch.manual_seed(3)
    a = m.sample(4)
    torch.manual_seed(3)
    assert torch.equal(m.sample(4), a) and tuple(a.shape) == (4, D) and bool(torch.isfinite(a).all())
    torch.manual_seed(3)
    zt = torch.randn(4, D, device=dev) * 0.5
    torch.manual_seed(3)
    assert torch.equal(m.sample(4, temperature=0.5), m.inverse(zt))
    for bad in (torch.zeros(B, D + 1, device=dev), torch.zeros(D, device=dev)):
        with pytest.raises(ValueError):
            m(bad)
        with pytest.raises(ValueError):
            m.inverse(bad)
        with pytest.raises(ValueError):
            m.log_prob(bad)
    with pytest.raises(ValueError):
        m.sample(3, z=zf[:2])
    with pytest.raises(ValueError):
        m.sample(2, temperature=0.0)


# ----------------------------------------------------------------------------------------------------------------------
# replay and capture
# ----------------------------------------------------------------------------------------------------------------------
FAST = (20, 5, 4, 24)      # D, B, layers, hidden of the replay tests


def _batches(dev, n):
    D, B, _, _ = FAST
    g = torch.Generator().manual_seed(9)
    return [(torch.rand(B, D, generator=g).mul(2).sub(1).to(dev), torch.zeros(B, dtype=torch.long, device=dev)) for _ in range(n)]


def _fast_net(dev):
    D, B, L, H = FAST
    return _net(D, L, H, NR.nice_init(D, L, H, 2602), dev, alternate=True, exact_logdet=True, lr=1e-2)


def _fast_run(dev, use_graph, accumulate, clip, n):
    m = _fast_net(dev)
    opt = m.configure_optimizers()
    if clip:
        opt.max_grad_norm = 0.05
    f = m.make_fast_step(opt, 1, use_graph, accumulate)
    losses = [f.step((x.clone(), c.clone()), i).detach().clone().reshape(()) for i, (x, c) in enumerate(_batches(dev, n))]
    st = opt._state(m._flat)
    return f, m, losses, (m._flat.data.clone(), st["m"].clone(), st["v"].clone())


def test_three_fast_steps_equal_eager_launches_to_the_bit(dev):
    from lgm_hip.optim import FusedAdam
    for clip in (False, True):
        f, m, la, sa = _fast_run(dev, True, 1, clip, 3)
        assert f.mode.startswith("hipGraph"), f.mode
        assert isinstance(f.opt, FusedAdam)
        b = _fast_net(dev)
        ob = b.configure_optimizers()
        if clip:
            ob.max_grad_norm = 0.05
        lb = []
        for i, (x, c) in enumerate(_batches(dev, 3)):
            loss = b.training_step((x, c), i)
            loss.backward()
            ob.step()
            ob.zero_grad()
            lb.append(loss.detach().clone().reshape(()))
        st = ob._state(b._flat)
        assert all(torch.equal(p, q) for p, q in zip(la, lb)), (clip, la, lb)
        assert torch.equal(sa[0], b._flat.data) and torch.equal(sa[1], st["m"]) and torch.equal(sa[2], st["v"]), clip
        assert float(la[0]) != float(la[2])
        assert torch.equal(m.logged["train_loss"].reshape(()), la[2]), "replay refreshes the logged scalar"
    # two micro-batches per optimizer step: the replayed step against the same step object issuing eager launches
    f, _, la, sa = _fast_run(dev, True, 2, False, 4)
    assert f.mode.startswith("hipGraph"), f.mode
    g, _, lb, sb = _fast_run(dev, False, 2, False, 4)
    assert not g.mode.startswith("hipGraph")
    assert all(torch.equal(p, q) for p, q in zip(la, lb)) and all(torch.equal(p, q) for p, q in zip(sa, sb))
    # ... and against plain training_step / backward / opt.step with no step object: the two micro-gradients are added and the
    # optimizer steps on their mean (a factor of 1/2 is exact, so where it is applied does not show in the bits)
    b = _fast_net(dev)
    ob = b.configure_optimizers()
    lc, micro = [], []
    for i, (x, c) in enumerate(_batches(dev, 4)):
        loss = b.training_step((x, c), i)
        b._flat.zero_grad()
        loss.backward()
        lc.append(loss.detach().clone().reshape(()))
        micro.append(b._flat.grad.clone())
        if i % 2 == 1:
            assert not torch.equal(micro[-2], micro[-1])
            b._flat.grad.copy_(micro[-2] + micro[-1])
            ob.grad_scale = 0.5
            ob.step()
            ob.zero_grad()
    st = ob._state(b._flat)
    assert all(torch.equal(p, q) for p, q in zip(la, lc)), (la, lc)
    assert torch.equal(sa[0], b._flat.data) and torch.equal(sa[1], st["m"]) and torch.equal(sa[2], st["v"])


# ----------------------------------------------------------------------------------------------------------------------
# train.py
# ----------------------------------------------------------------------------------------------------------------------
def test_train_entry_runs_nice_on_graph_replay(dev, tmp_path):
    """train.py's main() on configs/flow/nice.json at a reduced size: a few graph-replayed steps, the loss finite and
    falling (first two steps against last two), samples finite; last.ckpt loads into a CPU NICE"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "flow", "nice.json")))
    cfg["dataset"].update(img_size=8, batch_size=8)
    cfg["model"]["args"].update(img_size=8, hidden_dim=32, lr=1e-2)
    path = tmp_path / "nice_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_nice"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; from models.generative.flow.nice import NICE; "
            "L = []; end = NICE.on_train_batch_end; "
            "NICE.on_train_batch_end = lambda s, o, b, i: (L.append(float(s.logged['train_loss'])), end(s, o, b, i))[1]; "
            "m = train.main(sys.argv[2:]); "
            "print('STEPS', m.global_step, m.trainer.fast.mode); print('LOSSES', *L); "
            "o = m._optimizers[0]; print('OPT', type(getattr(o, '_opt', o)).__name__); "
            "s = m.sample(4); print('SAMPLE', tuple(s.shape), bool(torch.isfinite(s).all()))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "12", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "LOSSES", "OPT", "SAMPLE"))}
    assert lines["STEPS"].startswith("STEPS 12 hipGraph replay"), lines
    assert lines["OPT"] == "OPT FusedAdam", lines
    assert lines["SAMPLE"] == "SAMPLE (4, 1, 8, 8) True", lines
    losses = [float(v) for v in lines["LOSSES"].split()[1:]]
    assert len(losses) == 12 and all(math.isfinite(v) for v in losses), losses
    assert sum(losses[-2:]) < sum(losses[:2]), losses
    sd = torch.load(os.path.join(pkg, "experiments", "NICE", exp, "last.ckpt"), map_location="cpu", weights_only=False)
    assert sd["global_step"] == 12 and list(sd["state_dict"].keys()) == NR.keys(4)
    from models.generative.flow.nice import NICE
    cpu = NICE(img_channels=1, img_size=8, hidden_dim=32, alternate=True, exact_logdet=True)
    cpu.load_state_dict(sd["state_dict"])
    x = torch.rand(8, 1, 8, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1
    P = {k: v.double() for k, v in sd["state_dict"].items()}
    want = NR.forward(P, x.double().reshape(8, -1), True, True)[0]
    assert abs(float(cpu.training_step((x, None), 0).detach()) - float(want["loss"])) / abs(float(want["loss"])) < 1e-5
    assert rel(cpu.log_prob(x), want["log_prob"]) < 1e-5
    assert float(cpu.scaling_layer.log_scale.abs().min()) > 0, "the scaling layer was trained"
