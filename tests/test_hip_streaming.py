"""GPU: the streaming kernels - fused Adam / RMSprop / EMA / fill / clamp (csrc/optim.hip), colsum, the weighted-MSE loss and
its VQ-VAE twin, activations, axpby, upsample, pixel-unshuffle, layout changes and posemb (csrc/elementwise.hip) - per element
against the float64 references of oracle/streaming.py, at the tolerances measured by tests/test_cpu_streaming_bounds.py.

Every output lives inside a NaN-filled buffer with 32 floats of guard on both sides; pitched operands have NaN in the slack;
for the in-place flat kernels everything from n up to the end of the buffer is NaN in every operand.  Guards, slack and
tails must stay NaN.  Every score goes through the ``parity`` fixture."""
import math

import pytest
import torch

from oracle import streaming as st

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


class Flat:
    """n floats inside a NaN buffer: 32 floats of guard, ``shift`` more in front (an unaligned view), and at least four
    NaN floats behind element n - 1 before the rear guard (the tail a four-wide kernel must not touch)"""

    def __init__(self, data, dev, n=None, shift=0):
        self.n = n = data.numel() if data is not None else n
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + (n + 3) // 4 * 4 + 4 + GUARD,), NAN, device=dev)
        self.view = self.buf[self.lo:self.lo + n]
        if data is not None:
            self.view.copy_(data.to(dev))

    def result(self):
        return self.view.detach().cpu().clone()

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


class Mat:
    """[*lead, cols] as the channel slice [off, off + cols) of a NaN-filled [*lead, pitch] buffer between two guards"""

    def __init__(self, lead, cols, dev, pitch=None, off=0, data=None):
        lead = tuple(lead)
        pitch = pitch or cols
        R = math.prod(lead)
        assert off + cols <= pitch
        self.buf = torch.full((GUARD + R * pitch + GUARD,), NAN, device=dev)
        self.mask = torch.zeros_like(self.buf, dtype=torch.bool)
        self.view = self._slice(self.buf, lead, pitch, off, cols, R)
        self._slice(self.mask, lead, pitch, off, cols, R).fill_(True)
        if data is not None:
            self.view.copy_(data.reshape(*lead, cols).to(dev))

    @staticmethod
    def _slice(buf, lead, pitch, off, cols, R):
        return buf[GUARD:GUARD + R * pitch].view(*lead, pitch)[..., off:off + cols]

    def result(self):
        return self.view.detach().cpu().contiguous()

    def intact(self):
        return bool(torch.isnan(self.buf[~self.mask]).all())


def judge(parity, case, got):
    for k, units in case.scores(got).items():
        parity(f"{case.name}: {k}", units, case.tol)


# ---- flat kernels ------------------------------------------------------------------------------------------------------------

def _run_adam(case, dev, step_dev=False, lo=0, hi=None):
    from lgm_hip import ops
    hp = case.hp
    p, g, m, v = (Flat(t, dev) for t in case.inputs)
    hi = case.n if hi is None else hi
    sd = torch.tensor([float(case.step)], device=dev) if step_dev else None
    ops.adam_step(p.view[lo:hi], g.view[lo:hi], m.view[lo:hi], v.view[lo:hi], hi - lo, hp["lr"], hp["betas"][0], hp["betas"][1],
                  st.ADAM_EPS, hp["wd"], 0 if step_dev else case.step, sd, hp["grad_scale"], hp["decoupled"])
    torch.cuda.synchronize()
    assert all(f.intact() for f in (p, g, m, v)), f"{case.name}: a guard or the NaN tail behind element n was written"
    assert st.exact_units(g.result(), case.inputs[1]) == 0.0, "the gradient is read-only"
    return {"p": p.result(), "m": m.result(), "v": v.result()}


def _adam_case(parity, dev, case):
    got = _run_adam(case, dev)
    judge(parity, case, got)
    again = _run_adam(case, dev, step_dev=True)
    for k in got:
        assert st.exact_units(again[k], got[k]) == 0.0, f"{case.name}: step_dev gives other bits of {k} than the host step"


@pytest.mark.parametrize("n", [n for n in st.FLAT_SIZES if n not in (1027, 3074)])
def test_adam_sizes(dev, parity, n):
    _adam_case(parity, dev, st.AdamCase(n, "ddpm", 2))


@pytest.mark.parametrize("n", [1027, 3074])
@pytest.mark.parametrize("config", list(st.ADAM_CONFIGS))
def test_adam_configurations(dev, parity, config, n):
    """p, m and v of one step from the same float32 state at steps 1, 2, 7, 1000 and 100000, host step and step_dev.
    Measured on an MI355X: with the complements and bias corrections formed from float32 betas (the kernel before the
    betas crossed the ABI as doubles) v scored 217.8 units at b2 = 0.999 and p / m / v 22.7 / 6.2 / 19.8 at b2 = 0.99;
    formed in doubles the worst over every configuration is p 4.9, m 2.5, v 4.2 (torch.optim.Adam in float32 on the CPU:
    5.0).  The tolerance is 26."""
    for step in st.ADAM_STEPS:
        _adam_case(parity, dev, st.AdamCase(n, config, step))


@pytest.mark.parametrize("config", ["ddpm", "adamw"])
def test_adam_slice_equals_whole_buffer(dev, config):
    """a slice call [1024, 3072) as FusedAdam.step_slice issues it: the bits of the same range of a whole-buffer call, and
    nothing outside the slice moves"""
    case = st.AdamCase(3074, config, 7)
    whole = _run_adam(case, dev)
    part = _run_adam(case, dev, lo=1024, hi=3072)
    for k, old in zip(("p", "m", "v"), (case.inputs[0], case.inputs[2], case.inputs[3])):
        assert st.exact_units(part[k][1024:3072], whole[k][1024:3072]) == 0.0, k
        assert st.exact_units(part[k][:1024], old[:1024]) == 0.0 and st.exact_units(part[k][3072:], old[3072:]) == 0.0, k


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-one-float"])
@pytest.mark.parametrize("n", st.FLAT_SIZES)
def test_rmsprop(dev, parity, n, shift):
    from lgm_hip import ops
    for config, hp in st.RMSPROP_CONFIGS.items():
        case = st.RmspropCase(n, config)
        p, g, sq = (Flat(t, dev, shift=shift) for t in case.inputs)
        ops.rmsprop_step(p.view, g.view, sq.view, n, hp["lr"], hp["alpha"], st.ADAM_EPS, hp["wd"], hp["grad_scale"])
        torch.cuda.synchronize()
        assert p.intact() and g.intact() and sq.intact()
        judge(parity, case, {"p": p.result(), "sq": sq.result()})


@pytest.mark.parametrize("n", st.FLAT_SIZES)
def test_ema_lerp(dev, parity, n):
    """w == 1 is the reference's copy: online, bit for bit; w == 0 leaves the shadow's bits.  (s + (o - s) * w, taken
    literally, failed both on an MI355X: it is not o at w == 1 and turns a shadow of -0.0 into 0.0 at w == 0.)"""
    from lgm_hip import ops
    for w in st.EMA_WEIGHTS:
        case = st.EmaCase(n, w)
        sh, on = (Flat(t, dev) for t in case.inputs)
        ops.ema_lerp(sh.view, on.view, w)
        torch.cuda.synchronize()
        assert sh.intact() and on.intact() and st.exact_units(on.result(), case.inputs[1]) == 0.0
        judge(parity, case, {"shadow": sh.result()})


@pytest.mark.parametrize("n", st.FLAT_SIZES)
def test_fill_and_clamp(dev, n):
    from lgm_hip import ops
    x = Flat(None, dev, n=n)
    ops.fill(x.view, -1.5)
    torch.cuda.synchronize()
    assert x.intact() and torch.equal(x.result(), torch.full((n,), -1.5))
    g = torch.Generator().manual_seed(n)
    data = 2.0 * torch.randn(n, generator=g)
    data[0::5], data[1::5], data[2::7] = -0.75, 1.25, -0.0        # values exactly at the bounds
    for lo, hi in ((-0.75, 1.25), (0.5, 0.5), (0.0, 0.0)):
        x = Flat(data, dev)
        ops.clamp_(x.view, lo, hi)
        torch.cuda.synchronize()
        assert x.intact() and torch.equal(x.result(), data.clamp(lo, hi)), (lo, hi)


def test_ema_update_copies_flat_storage_before_update_after_step(dev):
    """EMA.update() at a step <= update_after_step is the reference's copy: every flat element of the shadow equals the
    online model afterwards"""
    from lgm_hip.optim import _first_flat
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(0)
    m = DDPM(img_channels=3, img_size=16, dim=16, lr=1e-3)
    m.to(dev)
    m.prepare_hip(dev)
    fo, fs = _first_flat(m.ema.online_model), _first_flat(m.ema.ema_model)
    assert fo is not None and fs is not None and fo.total == fs.total
    g = torch.Generator().manual_seed(1)
    on = torch.randn(fo.total, generator=g) * 10.0 ** (torch.rand(fo.total, generator=g) * 6 - 4)
    fo.data.copy_(on.to(dev))
    fs.data.copy_(torch.randn(fo.total, generator=g).to(dev))
    assert m.ema._step_py <= m.ema.update_after_step
    m.ema.update()
    torch.cuda.synchronize()
    assert st.exact_units(fs.data.cpu(), on) == 0.0 and st.exact_units(fo.data.cpu(), on) == 0.0


# ---- colsum ------------------------------------------------------------------------------------------------------------------

def _run_colsum(case, dev, deferred):
    from lgm_hip import ops
    rows, cols = case.rows, case.cols
    a = Mat((rows,), cols, dev, pitch=cols + 5, off=1, data=case.a)
    out = Flat(case.out0 if case.beta != 0.0 else None, dev, n=cols)       # beta == 0: onto NaN
    if deferred:
        queue = []
        ops.colsum(a.view, out.view.data_ptr(), case.beta, defer=queue)
        assert len(queue) == 1, "the deferred form was not taken"
        ops.wgrad_reduce_batch(queue, dev)
    else:
        ops.colsum(a.view, out.view.data_ptr(), case.beta)
    torch.cuda.synchronize()
    assert a.intact() and out.intact()
    return {"out": out.result()}


@pytest.mark.parametrize("shape", st.COLSUM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_colsum(dev, parity, shape):
    for beta in st.COLSUM_BETAS:
        case = st.ColsumCase(*shape, beta)
        got = _run_colsum(case, dev, deferred=False)
        judge(parity, case, got)
        if shape[1] % 4 == 0:
            d1, d2 = _run_colsum(case, dev, deferred=True), _run_colsum(case, dev, deferred=True)
            assert st.exact_units(d1["out"], d2["out"]) == 0.0, f"{case.name}: two deferred runs differ"
            assert st.exact_units(d1["out"], got["out"]) == 0.0, f"{case.name}: the deferred form gives other bits than the direct one"


# ---- weighted MSE and tanh_mse -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", st.MSE_SHAPES, ids=lambda s: "B{}-C{}-HW{}-Cp{}".format(*s))
def test_weighted_mse(dev, parity, shape):
    from lgm_hip import ops
    B, C, HW, Cpad = shape
    L = ops.lib()
    for weighted in (True, False):
        case = st.MseCase(*shape, weighted=weighted)
        o = Mat((B, HW), Cpad, dev, pitch=Cpad + 4, data=case.out)
        g = Mat((B, HW), Cpad, dev, pitch=Cpad + 4, data=case.tgt)
        gout = Mat((B, HW), Cpad, dev, pitch=Cpad + 4)
        per, loss = Flat(None, dev, n=B), Flat(None, dev, n=1)
        t, lw = case.t.to(dev), case.lw.to(dev)
        gloss = torch.tensor([case.gloss], device=dev)
        lwp = lw.data_ptr() if weighted else None
        L.lgm_weighted_mse_fwd(o.view.data_ptr(), g.view.data_ptr(), Cpad + 4, t.data_ptr(), lwp, B, C, HW, Cpad,
                               per.view.data_ptr(), loss.view.data_ptr(), ops.stream())
        L.lgm_weighted_mse_bwd(o.view.data_ptr(), g.view.data_ptr(), Cpad + 4, t.data_ptr(), lwp, gloss.data_ptr(), B, C, HW,
                               Cpad, gout.view.data_ptr(), ops.stream())
        torch.cuda.synchronize()
        assert all(b.intact() for b in (o, g, gout, per, loss))
        judge(parity, case, {"per_sample": per.result(), "loss": loss.result(), "gout": gout.result()})


@pytest.mark.parametrize("shape", st.MSE_SHAPES, ids=lambda s: "B{}-C{}-HW{}-Cp{}".format(*s))
def test_tanh_mse(dev, parity, shape):
    from lgm_hip import ops
    B, C, HW, Cpad = shape
    L = ops.lib()
    case = st.TanhMseCase(*shape)
    pre = Mat((B, HW), Cpad, dev, pitch=Cpad + 4, data=case.pre)
    tg = Mat((B, HW), Cpad, dev, pitch=Cpad + 4, data=case.tgt)
    xh, gpre = Mat((B, HW), Cpad, dev, pitch=Cpad + 4), Mat((B, HW), Cpad, dev, pitch=Cpad + 4)
    xh_in = Mat((B, HW), Cpad, dev, pitch=Cpad + 4, data=case.xh32)
    per, g2 = Flat(None, dev, n=B), Flat(None, dev, n=2)
    gloss = torch.tensor([case.gloss], device=dev)
    L.lgm_tanh_mse_fwd(pre.view.data_ptr(), tg.view.data_ptr(), Cpad + 4, B, C, HW, Cpad, xh.view.data_ptr(),
                       per.view.data_ptr(), ops.stream())
    L.lgm_tanh_mse_bwd(xh_in.view.data_ptr(), tg.view.data_ptr(), Cpad + 4, gloss.data_ptr(), case.w_recon, case.w_vq, B, C, HW,
                       Cpad, gpre.view.data_ptr(), g2.view.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in (pre, tg, xh, gpre, xh_in, per, g2))
    judge(parity, case, {"xh": xh.result(), "per_sample": per.result(), "gpre": gpre.result(), "g2": g2.result()})


# ---- activations and axpby ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", st.ACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("act", st.ACTS)
def test_activations(dev, parity, act, shape):
    """y = act(x + bias) + res and gx = (acc ? gx : 0) + gy act'(x + bias): bias on / off, residual on / off with its own pitch,
    accumulate on / off; inputs hold 0, -0.0, +-1e-8, +-1.2785, +-20, +-100 (no NaN or inf may appear: the score of a
    non-finite result is inf)"""
    from lgm_hip import ops
    code = {"silu": ops.ACT_SILU, "gelu": ops.ACT_GELU, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU, "tanh": ops.ACT_TANH}[act]
    rows, cols = shape
    for case in st.act_cases((act,), (shape,)):
        x = Mat((rows,), cols, dev, pitch=cols + 4, data=case.x)
        keep = case.b.to(dev) if case.bias else None                 # alive across the launch
        bias = keep.data_ptr() if case.bias else None
        if case.direction == "fwd":
            res = Mat((rows,), cols, dev, pitch=cols + 8, off=4, data=case.r) if case.res else None
            y = Mat((rows,), cols, dev, pitch=cols + 12, off=8)
            ops.act_fwd(x.view, bias, res.view if res else None, y.view, code, st.SLOPE)
            torch.cuda.synchronize()
            assert x.intact() and y.intact() and (res is None or res.intact())
            judge(parity, case, {"y": y.result()})
        else:
            gy = Mat((rows,), cols, dev, pitch=cols + 8, off=4, data=case.gy)
            gx = Mat((rows,), cols, dev, pitch=cols + 12, off=8, data=case.gx0 if case.acc else None)
            ops.act_bwd(x.view, bias, gy.view, gx.view, case.acc, code, st.SLOPE)
            torch.cuda.synchronize()
            assert x.intact() and gy.intact() and gx.intact()
            judge(parity, case, {"gx": gx.result()})


@pytest.mark.parametrize("shape", st.ACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_axpby(dev, parity, shape):
    from lgm_hip import ops
    rows, cols = shape
    for alpha, beta in st.AXPBY_COEFFS:
        for with_b in (True, False):
            case = st.AxpbyCase(rows, cols, alpha, beta, with_b)
            for in_place in (False, True):          # y is a: the form the residual paths of ddpm.py use
                a = Mat((rows,), cols, dev, pitch=cols + 4, data=case.a)
                b = Mat((rows,), cols, dev, pitch=cols + 8, off=4, data=case.b) if with_b else None
                y = a if in_place else Mat((rows,), cols, dev, pitch=cols + 12, off=8)
                ops.axpby(a.view, alpha, b.view if b else None, beta, y.view)
                torch.cuda.synchronize()
                assert a.intact() and y.intact() and (b is None or b.intact())
                judge(parity, case, {"y": y.result()})


# ---- spatial and layout kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", st.SPATIAL_C)
def test_upsample2x(dev, parity, C):
    from lgm_hip import ops
    B, H, W = st.SPATIAL["B"], st.SPATIAL["H"], st.SPATIAL["W"]
    g = torch.Generator().manual_seed(C)
    xs = torch.randn(B, H, W, C, generator=g)
    x = Mat((B, H, W), C, dev, pitch=C + 8, off=4, data=xs)
    y = Mat((B, 2 * H, 2 * W), C, dev, pitch=C + 12, off=8)
    ops.upsample2x_fwd(x.view, y.view)
    torch.cuda.synchronize()
    assert x.intact() and y.intact() and torch.equal(y.result(), st.upsample2x_fwd(xs))
    for acc in (False, True):
        case = st.UpsampleBwdCase(C, acc)
        gy = Mat((B, 2 * H, 2 * W), C, dev, pitch=C + 12, off=8, data=case.gy)
        gx = Mat((B, H, W), C, dev, pitch=C + 8, off=4, data=case.gx0 if acc else None)
        ops.upsample2x_bwd(gy.view, gx.view, acc)
        torch.cuda.synchronize()
        assert gy.intact() and gx.intact()
        judge(parity, case, {"gx": gx.result()})


@pytest.mark.parametrize("C", st.SPATIAL_C)
def test_pixel_unshuffle(dev, parity, C):
    from lgm_hip import ops
    B, H, W = st.SPATIAL["B"], st.SPATIAL["H"], st.SPATIAL["W"]
    g = torch.Generator().manual_seed(C + 1)
    his = torch.randn(B, 2 * H, 2 * W, C, generator=g)
    hi = Mat((B, 2 * H, 2 * W), C, dev, pitch=C + 3, off=1, data=his)
    lo = Mat((B, H, W), 4 * C, dev, pitch=4 * C + 8, off=4)
    ops.pixel_unshuffle(hi.view, lo.view, inverse=False)
    torch.cuda.synchronize()
    assert hi.intact() and lo.intact() and torch.equal(lo.result(), st.pixel_unshuffle(his))
    back = Mat((B, 2 * H, 2 * W), C, dev, pitch=C + 3, off=1)
    ops.pixel_unshuffle(back.view, lo.view, inverse=True)
    torch.cuda.synchronize()
    assert back.intact() and lo.intact() and torch.equal(back.result(), his)
    case = st.UnshuffleAccCase(C)
    lo = Mat((B, H, W), 4 * C, dev, pitch=4 * C + 8, off=4, data=case.lo)
    hi = Mat((B, 2 * H, 2 * W), C, dev, pitch=C + 3, off=1, data=case.hi0)
    ops.pixel_unshuffle(hi.view, lo.view, inverse=True, accumulate=True)
    torch.cuda.synchronize()
    assert hi.intact() and lo.intact()
    judge(parity, case, {"hi": hi.result()})


@pytest.mark.parametrize("C,Cpad", [(3, 4), (1, 4), (5, 8)])
def test_layout_round_trip(dev, C, Cpad):
    """nchw_to_nhwc into a pitched buffer: pad channels exactly 0, slack untouched; then back"""
    from lgm_hip import ops
    B, H, W = st.SPATIAL["B"], st.SPATIAL["H"], st.SPATIAL["W"]
    g = torch.Generator().manual_seed(C * 8 + Cpad)
    src = torch.randn(B, C, H, W, generator=g)
    srcd = src.to(dev)
    dst = Mat((B, H, W), Cpad, dev, pitch=Cpad + 3, off=1)
    ops.nchw_to_nhwc(srcd, dst.view)
    torch.cuda.synchronize()
    assert dst.intact() and torch.equal(dst.result().reshape(B, H * W, Cpad), st.nchw_to_nhwc(src, Cpad))
    back = Flat(None, dev, n=B * C * H * W)
    ops.nhwc_to_nchw(dst.view, back.view.view(B, C, H, W))
    torch.cuda.synchronize()
    assert back.intact() and dst.intact() and torch.equal(back.result().view(B, C, H, W), src)


# ---- posemb ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", st.POSEMB_SHAPES, ids=lambda s: "B{}-dim{}-pitch{}".format(*s))
def test_posemb(dev, parity, shape):
    from lgm_hip import ops
    B, dim, pitch = shape
    case = st.PosembCase(B, dim)
    assert torch.equal(ops.posemb_freqs(dim, st.POSEMB_THETA, dev).cpu(), case.freqs), "the host frequency table is the contract"
    out = Mat((B,), dim, dev, pitch=pitch)
    t = case.t.to(dev)
    ops.posemb(t, dim, st.POSEMB_THETA, out.view)
    torch.cuda.synchronize()
    assert out.intact()
    judge(parity, case, {"emb": out.result()})
