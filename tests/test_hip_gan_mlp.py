"""The MLP GAN on the GPU (csrc/bn1d.hip, lgm_hip.bn.BatchNorm1d, models/generative/gan/gan.py, lgm_hip.graph.GANFastStep).

Kernels per element against float64 under (k + 2) u M, u = 2^-24, as tests/test_hip_vae.py bounds its heads: M is the sum of
the absolute values that enter an element, k the roundings on the longest path (counted, not measured).  A
correctly rounded operation counts 1 (+, *, /, sqrtf), expf 1 ULP = 2, log1pf 2 ULP = 4.  With c = ceil(B / 16) (rows per
row group; the first addition to 0 is exact) and the 16 groups added in order:
  mean            c - 1 + 15 additions, the quotient: k = c + 15, M = sum_b |a| / B.
  rstd            a common error of the mean shifts every d = a - mean alike and leaves sum d^2 unchanged to first order
                  (sum d = 0); d 1 (relative to |d|), d^2 1, the sums c + 14, the quotient 1, + eps 1: k_var = c + 18 relative,
                  halved by the root; sqrtf 1, the reciprocal 1, one for the second-order term: k = ceil((c + 19) / 2) + 3,
                  M = rstd.
  y               gamma rstd d + beta.  The mean's error enters through d with weight |gamma| rstd (k = c + 15 on
                  M1 = |gamma| rstd sum |a| / B); on M2 = |gamma xhat|: d 1, rstd above, two products; the final sum 1 on
                  M2 + |beta|; LeakyReLU 1.  k = c + 18 (+ 1 with the activation), M = M1 + M2 + |beta|.  A one-pass variance
                  E[x^2] - E[x]^2 misses this bound at column means of 30 (tests/test_gan_host.py has the float64 side).
  running_mean    momentum mean 1 more, keep rm 1 (keep = 1 - momentum as the kernel rounds it), the sum 1: k = c + 17,
                  M = |keep rm| + momentum M_mean.
  running_var     var c + 18, B / (B - 1) 1, two products, the sum 1, the second-order term 1: k = c + 23,
                  M = |keep rv| + momentum var B / (B - 1).
  eval y          d 1, rstd (1 / 2 + 2 -> 3), two products, the sum, LeakyReLU: k = 8, M = |gamma xhat| + |beta|.
  backward        from the saved float32 mean and rstd, which the float64 side takes as given: g 1 (LeakyReLU'), xhat 2.
                  s1: k = c + 15, M = sum |g|;  s2: g xhat 3 more: k = c + 18, M = sum |g xhat|;  gbeta / ggamma: + 2 (beta_acc).
                  ga = (gamma rstd) ((g - s1 / B) - xhat (s2 / B)): the longest path is s2 (c + 18), / B 1, xhat 2, product 1,
                  two differences 2, gamma rstd 1, product 1: k = c + 26,
                  M = |gamma rstd| (|g| + sum |g| / B + |xhat| sum |g xhat| / B).
  bce losses      per sample expf 2, log1pf 4 + the propagated 2 (e / ((1 + e) log1p(e)) <= 1), the sum 1: 7 on
                  M_b = |max(s, 0) - s t| + log1p(e^-|s|) (s t is exact for t in {0, 1}); ceil(B / 64) additions per lane, the
                  wave tree 6, the quotient 1: k = 14 + ceil(B / 64), M = sum M_b / B; d_loss one more.  Mean logits
                  k = ceil(B / 64) + 7, M = sum |s| / B.
  bce gradients   sigmoid without cancellation (t = 1: -sigmoid(-s)): expf 2, 1 + e at most 2, the quotient 1: 5; the
                  coefficient gloss f / B 2, the product 1: k = 8, M = |gloss f (sigmoid(s) - t) / B|.

Buffers: NaN in every pad lane of the inputs and in guard rows and lanes around every buffer (which must stay NaN), exact-zero
pad lanes in the outputs, equal bits on a second run and at CU margins 0 and 16.  Both ``BatchNorm1d.route``s through the
module at the project's 1e-4.  The whole network against tests/golden/gan_mlp.npz (tools/make_golden_gan.py) under every
Linear and BatchNorm1d route, the graph-replayed step against eager ``_common_step``s to the bit, the no-tape paths, train.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gan_ref as GR

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24
NAN = float("nan")
SL = float(np.float32(0.2))                      # slope, eps and momentum as the kernels receive them
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
KEEP = float(np.float32(1.0) - np.float32(0.1))
ACT_NONE, ACT_LRELU = 0, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "gan_mlp.npz")))


def _ops():
    from lgm_hip import ops
    return ops


def _r4(n):
    return (n + 3) // 4 * 4


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a.reshape(-1) - b.reshape(-1)).norm() / b.norm().clamp_min(1e-30))


def _guarded(dev, B, C):
    """A [B, C] view inside a NaN-filled buffer with one guard row above and below and 4 guard lanes on each side"""
    buf = torch.full((B + 2, C + 8), NAN, device=dev)
    return buf[1:B + 1, 4:4 + C], buf


def _intact(buf, B, C):
    t = buf.clone()
    t[1:B + 1, 4:4 + C] = NAN
    return bool(torch.isnan(t).all())


def _vec(dev, v=None, n=None):
    """[n] inside NaN guards (no padding: the kernels take [F] vectors)"""
    n = v.numel() if v is not None else n
    buf = torch.full((n + 8,), NAN, device=dev)
    if v is not None:
        buf[4:4 + n] = v.to(dev)
    return buf[4:4 + n], buf


def _vec_intact(buf):
    return bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[-4:]).all())


def _input(dev, a):
    """[B, F] -> a view with pitch r4(F) + 8 whose pad lanes [F, r4(F)), guard lanes and guard rows hold NaN"""
    B, F = a.shape
    v, buf = _guarded(dev, B, _r4(F))
    v[:, :F] = a.to(dev)
    return v[:, :F]


def _margins(L, run):
    out = []
    try:
        for m in (0, 16):
            L.lgm_set_cu_margin(m)
            out.append(run())
    finally:
        L.lgm_set_cu_margin(-1)
    return out


class _Worst:
    """The worst measured value per quantity over the cases of one test.  ``report`` holds each against its tolerance through
    the ``parity`` recorder, with the case it came from: every case is still bounded (the worst is), and the record keeps one
    line per quantity and test."""

    def __init__(self):
        self.worst = {}

    def add(self, what, case, val, tol):
        val = float(val)
        if val != val:
            val = float("inf")                   # a NaN is a miss, never "not larger"
        cur = self.worst.get(what)
        if cur is None or val / tol > cur[0] / cur[2]:
            self.worst[what] = (val, case, tol)

    def report(self, parity, tag):
        for what, (val, case, tol) in self.worst.items():
            parity(f"{tag}: {what}" + (f" (worst at {case})" if case else ""), val, tol)


def _within(got, want, mag, k, what, case, acc):
    err = np.abs(np.asarray(torch.as_tensor(got).detach().double().cpu()) - np.asarray(want))
    bound = (k + 2) * U * np.maximum(np.asarray(mag), 1e-300)
    acc.add(what + " [|err| / ((k + 2) u M)]", f"{case}, k = {k}".lstrip(", "), float((err / bound).max()), 1.0)


_ids = lambda s: "x".join(map(str, s))      # noqa: E731


def _bn_operands(B, F, offset):
    g = torch.Generator().manual_seed(100 * B + F + int(offset))
    a = torch.randn(B, F, generator=g) + offset + (torch.randn(F, generator=g) if offset else 0.0)
    gamma, beta = torch.rand(F, generator=g) + 0.5, torch.rand(F, generator=g) - 0.5
    rm, rv = torch.rand(F, generator=g) - 0.5, torch.rand(F, generator=g) + 0.5
    return a.float(), gamma, beta, rm, rv


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm1d kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GR.BN_SHAPES, ids=_ids)
def test_bn1d_forward_per_element(dev, parity, shape):
    ops = _ops()
    L = ops.lib()
    B, F = shape
    Fp, c = _r4(F), -(-B // 16)
    acc = _Worst()
    for offset in (0.0, 30.0):                   # column means of about 30, unit spread: the centred variance's case
        a, gamma, beta, rm0, rv0 = _bn_operands(B, F, offset)
        a64, g64, b64 = a.double(), gamma.double(), beta.double()
        n64, xhat64, mean64, var64, rstd64 = GR.bn_train(a64, g64, b64, EPS)
        absmean = a64.abs().mean(0)
        M_y = g64.abs() * rstd64 * absmean + (g64 * xhat64).abs() + b64.abs()
        unb = var64 * B / (B - 1)
        av = _input(dev, a)
        gm, gm_buf = _vec(dev, gamma)
        bt, bt_buf = _vec(dev, beta)

        def run(act, training):
            yv, ybuf = _guarded(dev, B, Fp)
            rm, rm_buf = _vec(dev, rm0)
            rv, rv_buf = _vec(dev, rv0)
            mean, mean_buf = _vec(dev, n=F)
            rstd, rstd_buf = _vec(dev, n=F)
            ops.bn1d_fwd(av, F, gm.data_ptr(), bt.data_ptr(), EPS, MOM, training, act, SL, rm, rv, yv, mean, rstd)
            torch.cuda.synchronize()
            assert _intact(ybuf, B, Fp), "guard rows or lanes of y written"
            assert all(_vec_intact(b) for b in (rm_buf, rv_buf, mean_buf, rstd_buf, gm_buf, bt_buf)), "vector guards written"
            return [t.clone() for t in (yv, mean, rstd, rm, rv)]

        tag = f"mean {offset:g}"
        for act, name in ((ACT_NONE, "none"), (ACT_LRELU, "lrelu")):
            y, mean, rstd, rm, rv = run(act, True)
            want = n64 if act == ACT_NONE else n64.where(n64 > 0, n64 * SL)
            _within(y[:, :F], want, M_y, c + 18 + (act != ACT_NONE), "y", f"{tag} {name}", acc)
            assert bool((y[:, F:] == 0).all()), "pad lanes of the output are exactly 0"
            assert all(torch.equal(p, q) for p, q in zip(run(act, True), (y, mean, rstd, rm, rv))), "a second run: same bits"
        _within(mean, mean64, absmean, c + 15, "mean", tag, acc)
        _within(rstd, rstd64, rstd64, math.ceil((c + 19) / 2) + 3, "rstd", tag, acc)
        _within(rm, KEEP * rm0.double() + MOM * mean64, (KEEP * rm0.double()).abs() + MOM * absmean, c + 17,
                "running_mean", tag, acc)
        _within(rv, KEEP * rv0.double() + MOM * unb, (KEEP * rv0.double()).abs() + MOM * unb, c + 23,
                "running_var (unbiased)", tag, acc)
        biased = KEEP * rv0.double() + MOM * var64                     # what a missing B / (B - 1) would give
        assert float(((rv.double().cpu() - biased).abs() / ((c + 25) * U * rv0.double())).max()) > 1.0
        # eval mode: the running statistics normalise and are not written
        y, mean, rstd, rm, rv = run(ACT_LRELU, False)
        re64 = 1.0 / torch.sqrt(rv0.double() + EPS)
        ne64 = g64 * ((a64 - rm0.double()) * re64) + b64
        _within(y[:, :F], ne64.where(ne64 > 0, ne64 * SL), (g64 * (a64 - rm0.double()) * re64).abs() + b64.abs(), 8,
                "eval y", tag, acc)
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and torch.equal(mean.cpu(), rm0)
        assert bool((y[:, F:] == 0).all())
    acc.report(parity, f"bn1d_fwd {_ids(shape)}")
    m0, m16 = _margins(L, lambda: run(ACT_LRELU, True))
    assert all(torch.equal(p, q) for p, q in zip(m0, m16)), "CU margins 0 and 16 give the same bits"
    if B == 2:                                   # one row cannot be normalised by its own statistics
        from lgm_hip._lib import LgmArgumentError
        with pytest.raises(LgmArgumentError):
            ops.bn1d_fwd(av[:1], F, gm.data_ptr(), bt.data_ptr(), EPS, MOM, True, ACT_NONE, SL, rm, rv, y, mean, rstd)


@pytest.mark.parametrize("shape", GR.BN_SHAPES, ids=_ids)
def test_bn1d_backward_per_element(dev, parity, shape):
    ops = _ops()
    L = ops.lib()
    B, F = shape
    Fp, c = _r4(F), -(-B // 16)
    acc = _Worst()
    for offset in (0.0, 30.0):
        a, gamma, _, gg0, gb0 = _bn_operands(B, F, offset)
        g = torch.Generator().manual_seed(7 * B + F)
        gy = torch.randn(B, F, generator=g)
        y0 = torch.randn(B, F, generator=g)
        y0 = torch.where(y0 >= 0, 1.0, -1.0) * (y0.abs() + 1e-3)                     # >= 1e-3 from the kink
        _, _, mean64, _, rstd64 = GR.bn_train(a.double(), gamma.double(), gamma.double(), EPS)
        mean32, rstd32 = mean64.float(), rstd64.float()                              # the saved statistics, as given
        av, gyv, yv = _input(dev, a), _input(dev, gy), _input(dev, y0)
        gm, gm_buf = _vec(dev, gamma)
        mn, mn_buf = _vec(dev, mean32)
        rs, rs_buf = _vec(dev, rstd32)
        xhat = (a.double() - mean32.double()) * rstd32.double()
        cg = gamma.double() * rstd32.double()

        def run(act, beta_acc):
            gav, gabuf = _guarded(dev, B, Fp)
            gg, gg_buf = _vec(dev, gg0)
            gb, gb_buf = _vec(dev, gb0)
            ops.bn1d_bwd(gyv, yv if act != ACT_NONE else None, av, F, mn, rs, gm.data_ptr(), act, SL, gav, gg.data_ptr(),
                         gb.data_ptr(), beta_acc)
            torch.cuda.synchronize()
            assert _intact(gabuf, B, Fp), "guard rows or lanes of ga written"
            assert all(_vec_intact(b) for b in (gg_buf, gb_buf, gm_buf, mn_buf, rs_buf)), "vector guards written"
            return [t.clone() for t in (gav, gg, gb)]

        tag = f"mean {offset:g}"
        for act, name in ((ACT_NONE, "none"), (ACT_LRELU, "lrelu")):
            g64 = gy.double() * (torch.where(y0 > 0, 1.0, SL).double() if act != ACT_NONE else 1.0)
            s1, s2 = g64.sum(0), (g64 * xhat).sum(0)
            A1, A2 = g64.abs().sum(0), (g64 * xhat).abs().sum(0)
            for beta_acc in (0.0, 1.0):
                ga, gg, gb = run(act, beta_acc)
                t = f"{tag} {name} beta_acc {beta_acc:g}"
                _within(gb, beta_acc * gb0.double() + s1, beta_acc * gb0.double().abs() + A1, c + 17, "gbeta", t, acc)
                _within(gg, beta_acc * gg0.double() + s2, beta_acc * gg0.double().abs() + A2, c + 20, "ggamma", t, acc)
                _within(ga[:, :F], cg * (g64 - s1 / B - xhat * s2 / B), cg.abs() * (g64.abs() + A1 / B + xhat.abs() * A2 / B),
                        c + 26, "ga", t, acc)
                assert bool((ga[:, F:] == 0).all()), "pad lanes of the output are exactly 0"
            assert all(torch.equal(p, q) for p, q in zip(run(act, 1.0), (ga, gg, gb))), "a second run: same bits"
    acc.report(parity, f"bn1d_bwd {_ids(shape)}")
    m0, m16 = _margins(L, lambda: run(ACT_LRELU, 1.0))
    assert all(torch.equal(p, q) for p, q in zip(m0, m16)), "CU margins 0 and 16 give the same bits"


@pytest.mark.parametrize("route", ["rows", "generic"])
@pytest.mark.parametrize("shape", [(3, 6), (17, 36), (33, 260), (130, 16), (600, 36)], ids=_ids)
def test_batchnorm1d_module_both_routes(dev, parity, monkeypatch, shape, route):
    """``BatchNorm1d.fwd`` / ``bwd`` on flat storage; (600, 36) is past what a strip holds and takes the two-launch pairs
    under either route; (3, 6) / F = 6: running statistics that are no multiple of 4 long"""
    from lgm_hip.bn import BatchNorm1d
    from lgm_hip.flat import FlatParams
    from lgm_hip.nn import GradCtx, param_kind
    ops = _ops()
    monkeypatch.setattr(BatchNorm1d, "route", route)
    B, F = shape
    a, gamma, beta, rm0, rv0 = _bn_operands(B, F, 30.0)
    bn = BatchNorm1d(F)
    bn.load_state_dict({"weight": gamma, "bias": beta, "running_mean": rm0, "running_var": rv0,
                        "num_batches_tracked": torch.tensor(5)})
    bn.to(dev)
    flat = FlatParams([(n, p, param_kind(n, p)) for n, p in bn.named_parameters()], dev)
    av = torch.zeros(B, _r4(F), device=dev)
    av[:, :F] = a.to(dev)
    n64, xhat64, mean64, var64, rstd64 = GR.bn_train(a.double(), gamma.double(), beta.double(), EPS)
    y, sv = bn.fwd(av[:, :F], ACT_LRELU, SL, True)
    assert (sv.a.dim() == 2) == (route == "rows" and B <= 512)
    t = f"BatchNorm1d {route} {_ids(shape)}"
    parity(f"{t}: y", rel(y[:, :F], n64.where(n64 > 0, n64 * SL)), RTOL)
    assert bool((y[:, F:] == 0).all())
    rm64, rv64 = GR.bn_running(rm0.double(), rv0.double(), mean64, var64, B, MOM)
    parity(f"{t}: running_mean", rel(bn.running_mean, rm64), RTOL)
    parity(f"{t}: running_var", rel(bn.running_var, rv64), RTOL)
    gy = torch.randn(B, F, generator=torch.Generator().manual_seed(3))
    gyv = torch.zeros(B, _r4(F), device=dev)
    gyv[:, :F] = gy.to(dev)
    flat.zero_grad()
    gc = GradCtx(flat, transposed=False)
    ga = bn.bwd(gc, sv, y, gyv, ACT_LRELU, SL)
    flat.bind_grad_views()
    ga64, gg64, gb64 = GR.bn_backward(gy.double() * GR.dlrelu(n64), xhat64, gamma.double(), rstd64)
    parity(f"{t}: ga", rel(ga[:, :F], ga64), RTOL)
    parity(f"{t}: ggamma", rel(bn.weight.grad, gg64), RTOL)
    parity(f"{t}: gbeta", rel(bn.bias.grad, gb64), RTOL)
    bn.eval()
    ye, _ = bn.fwd(av[:, :F], ACT_NONE, 0.0, False)
    parity(f"{t}: eval y", rel(ye[:, :F], GR.bn_eval(a.double(), gamma.double(), beta.double(), rm64, rv64, EPS)), RTOL)
    assert int(bn.state_dict()["num_batches_tracked"]) == 6, "one train-mode forward, none for eval"
    bn.train()
    with pytest.raises(ValueError):
        bn.fwd(av[:1, :F], ACT_NONE, 0.0, True)


# ----------------------------------------------------------------------------------------------------------------------
# the loss head
# ----------------------------------------------------------------------------------------------------------------------
def _scores(B):
    g = torch.Generator().manual_seed(B)
    if B < 5:
        return [torch.full((B,), v) for v in (40.0, -40.0, 0.0)]
    s = torch.randn(B, generator=g) * 3
    s[:3] = torch.tensor([40.0, -40.0, 0.0])
    s2 = torch.randn(B, generator=g) * 3
    s2[-3:] = torch.tensor([0.0, 40.0, -40.0])
    return [s, s2]


def _score_matrix(dev, s):
    v, buf = _guarded(dev, s.numel(), 4)         # the dense head's [B, 4]: lanes 1 .. 3 are never read
    v[:, 0] = s.to(dev)
    return v


@pytest.mark.parametrize("B", GR.BCE_SIZES)
def test_bce_kernels_per_element(dev, parity, B):
    ops = _ops()
    cb = -(-B // 64)
    acc = _Worst()
    vecs = _scores(B)
    for i, s in enumerate(vecs):
        f = vecs[(i + 1) % len(vecs)]
        s64, f64 = s.double(), f.double()
        sv, fv = _score_matrix(dev, s), _score_matrix(dev, f)
        Mr = (s64.clamp_min(0) - s64).abs() + torch.log1p(torch.exp(-s64.abs()))
        Mf = f64.clamp_min(0) + torch.log1p(torch.exp(-f64.abs()))
        vals, vbuf = _vec(dev, n=5)
        ops.gan_bce_d(sv, fv, vals)
        torch.cuda.synchronize()
        assert _vec_intact(vbuf)
        real, fake = GR.bce(s64, 1.0).mean(), GR.bce(f64, 0.0).mean()
        t = f"scores #{i}"
        _within(vals[0], real, Mr.mean(), 14 + cb, "d_loss_real", t, acc)
        _within(vals[1], fake, Mf.mean(), 14 + cb, "d_loss_fake", t, acc)
        _within(vals[2], (real + fake) / 2, (Mr.mean() + Mf.mean()) / 2, 15 + cb, "d_loss", t, acc)
        _within(vals[3], s64.mean(), s64.abs().mean(), cb + 7, "mean logit", f"{t} real", acc)
        _within(vals[4], f64.mean(), f64.abs().mean(), cb + 7, "mean logit", f"{t} fake", acc)
        again, _ = _vec(dev, n=5)
        ops.gan_bce_d(sv, fv, again)
        assert torch.equal(again, vals), "a second run gives the same bits"
        for lt in GR.LOSS_TYPES:
            v2, v2buf = _vec(dev, n=2)
            ops.gan_bce_g(sv, lt, v2)
            torch.cuda.synchronize()
            assert _vec_intact(v2buf)
            want = real if lt == "non-saturating" else -GR.bce(s64, 0.0).mean()
            M = Mr.mean() if lt == "non-saturating" else (s64.clamp_min(0) + torch.log1p(torch.exp(-s64.abs()))).mean()
            _within(v2[0], want, M, 14 + cb, f"g_loss {lt}", t, acc)
            _within(v2[1], s64.mean(), s64.abs().mean(), cb + 7, "mean logit", f"{t} {lt}", acc)
        # gradients, gloss != 1
        gl = torch.tensor([0.37], device=dev)
        gl64 = float(np.float32(0.37))
        g0, g0buf = _guarded(dev, B, 4)
        g1, g1buf = _guarded(dev, B, 4)
        ops.gan_bce_bwd(gl, sv, 1.0, 0.5, g0, fv, 0.0, 0.5, g1)
        torch.cuda.synchronize()
        assert _intact(g0buf, B, 4) and _intact(g1buf, B, 4)
        w0 = gl64 * 0.5 * -torch.sigmoid(-s64) / B                                  # sigmoid(s) - 1 without cancellation
        w1 = gl64 * 0.5 * torch.sigmoid(f64) / B
        _within(g0[:, 0], w0, w0.abs(), 8, "score gradient", f"{t} d real", acc)
        _within(g1[:, 0], w1, w1.abs(), 8, "score gradient", f"{t} d fake", acc)
        assert bool((g0[:, 1:] == 0).all()) and bool((g1[:, 1:] == 0).all())
        for lt, tt, ff, w in (("non-saturating", 1.0, 1.0, gl64 * -torch.sigmoid(-s64) / B),
                              ("min-max", 0.0, -1.0, -gl64 * torch.sigmoid(s64) / B)):
            g2, g2buf = _guarded(dev, B, 4)
            ops.gan_bce_bwd(gl, sv, tt, ff, g2)
            torch.cuda.synchronize()
            assert _intact(g2buf, B, 4) and bool((g2[:, 1:] == 0).all())
            _within(g2[:, 0], w, w.abs(), 8, "score gradient", f"{t} {lt}", acc)
    acc.report(parity, f"gan_bce B {B}")


# ----------------------------------------------------------------------------------------------------------------------
# the whole network
# ----------------------------------------------------------------------------------------------------------------------
def _net(fx, case, dev, **kw):
    from models.generative.gan.gan import GAN
    C, S, L, B = fx[f"{case}:dims"].tolist()
    m = GAN(C, S, L, **kw)
    m.load_state_dict(GR.gan_init(C, S, L, int(fx[f"{case}:seed"])))
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


ROUTES = {"dense+rows": ("dense", "dense", "rows"), "generic+rows": ("generic", "generic", "rows"),
          "generic_bwd+rows": ("dense", "generic", "rows"), "dense+generic": ("dense", "dense", "generic"),
          "generic+generic": ("generic", "generic", "generic")}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", ["a", "b"])
def test_whole_network_against_the_reference_fixture(fx, dev, parity, monkeypatch, case, route):
    from lgm_hip.bn import BatchNorm1d
    from lgm_hip.nn import Linear
    fwd_r, bwd_r, bn_r = ROUTES[route]
    monkeypatch.setattr(Linear, "fwd_route", fwd_r)
    monkeypatch.setattr(Linear, "bwd_route", bwd_r)
    monkeypatch.setattr(BatchNorm1d, "route", bn_r)
    m = _net(fx, case, dev)
    C, S, L, B = fx[f"{case}:dims"].tolist()
    x, z = torch.from_numpy(fx[f"{case}:x"]).to(dev), torch.from_numpy(fx[f"{case}:z"]).to(dev)
    t, acc = f"case {case} {route}", _Worst()
    x_hat = m.G(z)
    assert tuple(x_hat.shape) == (B, C, S, S) and x_hat.requires_grad
    acc.add("x_hat", "", rel(x_hat, fx[f"{case}:x_hat"]), RTOL)
    sd = m.G.state_dict()
    for k in sd:
        if "running" in k:
            acc.add("running statistics", k, rel(sd[k], fx[f"{case}:G.{k}"]), RTOL)
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 1
    acc.add("logits", "real", rel(m.D(x), fx[f"{case}:s_real"]), RTOL)
    acc.add("logits", "fake", rel(m.D(x_hat.detach()), fx[f"{case}:s_fake"]), RTOL)
    d = m._calculate_d_loss(x, x_hat)
    assert list(d) == ["d_loss", "d_loss_real", "d_loss_fake", "logits_real", "logits_fake"]
    m.D._flat.zero_grad()
    d["d_loss"].backward()
    torch.cuda.synchronize()
    for k in d:
        acc.add("d losses and mean logits", k, rel(d[k], fx[f"{case}:{k}"]), RTOL)
    for n, p in m.D.named_parameters():
        acc.add("grad D", n, GR.fixture_grad_error(fx, case, f"D.{n}", p.grad), RTOL)
    d_grads = m.D._flat.grad.clone()
    for lt in GR.LOSS_TYPES:
        m.hparams["loss_type"] = lt
        xh = m.G(z)                                      # a new tape (a backward consumes it); the same batch statistics
        assert torch.equal(xh, x_hat)
        g = m._calculate_g_loss(xh)
        assert list(g) == ["g_loss", "logits_fake"]
        m.G._flat.zero_grad()
        g["g_loss"].backward()
        torch.cuda.synchronize()
        acc.add(f"{lt}: g_loss", "", rel(g["g_loss"], fx[f"{case}:g_loss:{lt}"]), RTOL)
        acc.add(f"{lt}: logits_fake", "", rel(g["logits_fake"], fx[f"{case}:logits_fake"]), RTOL)
        grads = dict(m.G.named_parameters())
        for n, p in grads.items():
            if n in ("model.0.bias", "model.3.bias", "model.6.bias"):
                # analytically zero: the BatchNorm behind the layer removes the column mean.  Absolute, not relative
                top = float(grads[n.replace("bias", "weight")].grad.abs().max())
                acc.add(f"{lt}: |zero bias grad| / max |gw|", n, float(p.grad.abs().max()) / top, 1e-4)
            else:
                acc.add(f"{lt}: grad G", n, GR.fixture_grad_error(fx, case, f"G:{lt}:{n}", p.grad), RTOL)
        assert torch.equal(m.D._flat.grad, d_grads), "the generator update forms no gradient of D"
    acc.report(parity, t)


def _batches(fx, case, dev, n):
    C, S, L, B = fx[f"{case}:dims"].tolist()
    g = torch.Generator().manual_seed(9)
    return [(torch.rand(B, C, S, S, generator=g).mul(2).sub(1).to(dev), torch.zeros(B, dtype=torch.long, device=dev))
            for _ in range(n)]


def _three_steps(fx, dev, how):
    """how: "replay" / "fast-eager" (the step object, use_graph off) / "module" (eager ``_common_step``s)"""
    from lgm_hip.lightning import _CountingOptimizer
    torch.manual_seed(21)
    torch.cuda.manual_seed(21)
    m = _net(fx, "b", dev, lr=1e-2)
    opts, _ = m.configure_optimizers()
    m._optimizers = [_CountingOptimizer(o, m) for o in opts]
    f = m.make_fast_step(m._optimizers, 1, how == "replay") if how != "module" else None
    logs = []
    for i, (x, c) in enumerate(_batches(fx, "b", dev, 3)):
        if f is not None:
            f.step((x.clone(), c.clone()), i)
        else:
            m.training_step((x, c))
        logs.append({k: v.detach().clone() for k, v in m.logged.items()})
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    adam = [o._opt._state(n._flat) for o, n in zip(m._optimizers, (m.D, m.G))]
    extra = [t.clone() for st in adam for t in (st["m"], st["v"])] + [m.G._flat.data.clone(), m.D._flat.data.clone()]
    return f, m, logs, state, extra, torch.randn(8, device=dev)


def test_three_fast_steps_equal_eager_common_steps_to_the_bit(fx, dev):
    from lgm_hip.optim import FusedAdam
    f, m, la, sa, ea, za = _three_steps(fx, dev, "replay")
    assert f.mode.startswith("hipGraph"), f.mode
    assert all(isinstance(o._opt, FusedAdam) for o in m._optimizers) and m.global_step == 6
    for how in ("module", "fast-eager"):
        g, b, lb, sb, eb, zb = _three_steps(fx, dev, how)
        assert g is None or not g.mode.startswith("hipGraph")
        assert b.global_step == 6
        for i in range(3):
            assert set(la[i]) == set(lb[i]) == {"train_d_loss", "train_d_loss_real", "train_d_loss_fake", "train_logits_real",
                                                "train_logits_fake", "train_g_loss"}
            assert all(torch.equal(la[i][k].reshape(()), lb[i][k].reshape(())) for k in la[i]), (how, i)
        assert list(sa) == list(sb) == GR.KEYS and all(torch.equal(sa[k], sb[k]) for k in sa), how
        assert all(torch.equal(p, q) for p, q in zip(ea, eb)), how
        assert torch.equal(za, zb), "the run that captures and the run that never tries draw the same z"
    assert int(sa["G.model.4.num_batches_tracked"]) == 3
    assert float(la[0]["train_d_loss"]) != float(la[2]["train_d_loss"])
    assert not torch.equal(sa["G.model.1.running_mean"], GR.gan_init(3, 5, 3, int(fx["b:seed"]))["G.model.1.running_mean"].to(dev))
    # a batch of another shape takes eager launches in the same object
    C, S, L, B = fx["b:dims"].tolist()
    out = f.step((torch.zeros(B + 1, C, S, S, device=dev), None), 3)
    assert bool(torch.isfinite(out["train_g_loss"])) and m.global_step == 8


def test_no_tape_paths_against_float64_and_the_refusals(fx, dev, parity):
    m = _net(fx, "a", dev)
    C, S, L, B = fx["a:dims"].tolist()
    P = GR.to64(GR.gan_init(C, S, L, int(fx["a:seed"])))
    z = torch.randn(7, L, generator=torch.Generator().manual_seed(4))
    m.eval()
    img = m.sample(7, z=z.to(dev))
    assert tuple(img.shape) == (7, C, S, S) and not img.requires_grad
    parity("sample (eval): x_hat", rel(img, GR.g_forward(P, z.double(), False)[0]), RTOL)
    with torch.no_grad():
        assert torch.equal(m(z.to(dev)), img) and torch.equal(m.G(z.to(dev)), img)
    one = m.sample(1, z=z[:1].to(dev))
    parity("sample (eval, one row)", rel(one, GR.g_forward(P, z[:1].double(), False)[0]), RTOL)
    assert int(m.state_dict()["G.model.1.num_batches_tracked"]) == 0
    m.train()
    xh64, _, running = GR.g_forward(P, z.double(), True)
    parity("sample (train): x_hat", rel(m.sample(7, z=z.to(dev)), xh64), RTOL)
    parity("sample (train): running_var", rel(m.G.model[7].running_var, running["G.model.7.running_var"]), RTOL)
    assert int(m.state_dict()["G.model.1.num_batches_tracked"]) == 1
    torch.manual_seed(3)
    a = m.sample(5)
    torch.manual_seed(3)
    assert torch.equal(m.sample(5), a) and tuple(a.shape) == (5, C, S, S) and float(a.abs().max()) <= 1.0
    for bad in (torch.zeros(3, L + 1, device=dev), torch.zeros(L, device=dev), torch.zeros(2, L, device=dev)):
        with pytest.raises(ValueError):
            m.sample(3, z=bad)
    with pytest.raises(ValueError):
        m.sample(1)                                      # train mode, one row
    with torch.no_grad():
        m.eval()
        from lgm_hip.lightning import _CountingOptimizer
        m._optimizers = [_CountingOptimizer(o, m) for o in m.configure_optimizers()[0]]
        m.validation_step((torch.from_numpy(fx["a:x"]).to(dev), None))
    assert bool(torch.isfinite(m.logged["val_g_loss"])) and m.global_step == 0


def test_train_entry_runs_the_gan_on_graph_replay(dev, tmp_path):
    """train.py's main() on configs/gan/gan.json at a reduced size (the synthetic-data route): a few graph-replayed steps;
    last.ckpt loads into a CPU GAN that takes a step"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "gan", "gan.json")))
    cfg["dataset"].update(img_size=8, batch_size=8)
    cfg["model"]["args"].update(img_size=8, latent_dim=6)
    path = tmp_path / "gan_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_gan"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('STEPS', m.global_step, m.trainer.fast.mode); print('G_LOSS', float(m.logged['train_g_loss'])); "
            "print('OPT', ' '.join(type(getattr(o, '_opt', o)).__name__ for o in m._optimizers))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "8", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "G_LOSS", "OPT"))}
    assert lines["STEPS"].startswith("STEPS 8 hipGraph replay"), lines             # two optimizer steps per batch
    assert lines["OPT"] == "OPT FusedAdam FusedAdam", lines
    assert np.isfinite(float(lines["G_LOSS"].split()[1]))
    sd = torch.load(os.path.join(pkg, "experiments", "GAN", exp, "last.ckpt"), map_location="cpu", weights_only=False)
    assert sd["global_step"] == 8 and list(sd["state_dict"].keys()) == GR.KEYS
    assert int(sd["state_dict"]["G.model.1.num_batches_tracked"]) == 4
    from lgm_hip.lightning import _CountingOptimizer
    from models.generative.gan.gan import GAN
    cpu = GAN(1, 8, 6)
    cpu.load_state_dict(sd["state_dict"])
    cpu._optimizers = [_CountingOptimizer(o, cpu) for o in cpu.configure_optimizers()[0]]
    cpu.train()
    out = cpu.training_step((torch.rand(8, 1, 8, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1, None))
    assert all(bool(torch.isfinite(v)) for v in out.values())
