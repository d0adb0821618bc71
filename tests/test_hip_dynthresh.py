"""GPU: dynamic thresholding of x0 in the samplers (``GaussianDiffusion(dynamic_thresholding=True)``; Saharia et al. 2022, 2.3,
an extension of the reference).

  * dyn_thresh_kernel alone: the selection bit for bit against a float32 restatement from ``torch.sort``, all objectives against
    float64, NaN in every lane it must not read, the table + counter form against the by-value form;
  * the update kernels with a threshold buffer against float64 (bounds below), |x0| <= 1, pad lanes, the history and the self-
    conditioning slice, in place against out of place, thresholds of one against the static-clip entry points bit for bit;
  * whole chains against tests/golden/diffusion_dynthresh.npz (tools/make_golden_dynthresh.py: loops around the REFERENCE's
    network and unclipped model_predictions), 1e-4 relative, a miss decided by the float64 arbiter rule of
    tests/test_hip_dpmpp.py; graph replay bit for bit against eager launches and against a second replay;
  * two percentiles on one network, static-clip chains beside thresholded ones, p_sample against p_mean_variance, dispatch
    through ``sample``, train.py on configs/diffusion/ddpm_cond_dynthresh.json.

Measured distances go through the ``parity`` recorder (committed record: profiles/r11_dynthresh_parity.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24                        # unit roundoff of float32
NAN = float("nan")
OBJ = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def unpack64(fx, key):
    """a float64 result of the fixture: the float32 one plus the stored int8 residual (tools/make_golden_dynthresh.py)"""
    return fx[key].astype(np.float64) + fx[key + ":r64"].astype(np.float64) * float(fx[key + ":r64_scale"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_dynthresh.npz")))


def _r4(n):
    return (n + 3) // 4 * 4


# ----------------------------------------------------------------------------------------------------------------------
# dyn_thresh_kernel alone.  One path for every n (three radix passes over the sample, whatever its size).
# ----------------------------------------------------------------------------------------------------------------------
GEOMS = [(3, 3, 25, 4, 0, -1),        # n = 75: fewer elements than threads, no multiple of 64
         (2, 3, 1024, 8, 3, 0),       # self-conditioned: slices at lanes 0 and 3 of a pitch of 8
         (2, 1, 64, 4, 0, -1),
         (2, 3, 16384, 4, 0, -1)]     # n = 49152: 48 elements per thread
GIDS = ["3x3x25", "selfcond_2x3x1024", "2x1x64", "2x3x16384"]
PERCENTILES = (0.5, 0.95, 0.995, 1.0)


@pytest.fixture(scope="module")
def heads():
    """(A, Bv, R, Rm1) of the sigmoid schedule at t = 999, 500, 0, and the solver / DDIM rows they head"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)
    grid = [(999, 750), (750, 500), (500, 250), (250, 0), (0, -1)]
    sde = sampler.dpm_coeffs(gd, grid, 2, True)
    dpm = {999: sde[0], 500: sde[2], 0: sde[4]}
    ddim = {999: sampler._ddim_coeffs(gd, 999, 750, 1.0), 500: sampler._ddim_coeffs(gd, 500, 250, 1.0),
            0: sampler._ddim_coeffs(gd, 0, -1, 1.0)}
    assert dpm[500][6] != 0.0 and dpm[500][7] != 0.0 and ddim[500][7] != 0.0 and all(dpm[t][:4] == ddim[t][:4] for t in dpm)
    return {"dpm": dpm, "ddim": ddim}


def _buffers(seed, geom, v_values=None):
    """host buffers with NaN wherever the kernels must not read: the pad lanes and the self-conditioning slice of the input
    buffer, the pad lanes of the network output.  ``v_values`` [B, HW, C]: the network output's real lanes."""
    B, C, HW, pitch, x_off, sc_off = geom
    g = torch.Generator().manual_seed(seed)
    xin = torch.full((B, HW, pitch), NAN)
    xin[..., x_off:x_off + C] = torch.randn(B, HW, C, generator=g) * 1.5
    v = torch.full((B, HW, _r4(C)), NAN)
    v[..., :C] = torch.randn(B, HW, C, generator=g) if v_values is None else v_values
    return xin, v


def _dyn(dev, geom, xin, v, objective, head, p, table=None, counter=None):
    from lgm_hip import ops, sampler
    B, C, HW, pitch, x_off, sc_off = geom
    k, w = sampler.dyn_rank(C * HW, p)
    s = torch.full((B,), NAN, device=dev)
    A, Bv, R, Rm1 = (0.0,) * 4 if head is None else head[:4]
    ops.lib().lgm_dyn_thresh(xin.data_ptr(), pitch, x_off, v.data_ptr(), v.shape[-1], B, C, HW, objective, A, Bv, R, Rm1,
                             None if table is None else table.data_ptr(), None if counter is None else counter.data_ptr(),
                             k, w, s.data_ptr(), ops.stream())
    assert ops.lib()._dll.lgm_last_kernel().decode() == "dyn_thresh_kernel"
    return s.cpu()


def _restated(a, k, w):
    """float32, separate operations: a [B, n] magnitudes -> max(lo + w (hi - lo), 1)"""
    srt = a.float().sort(dim=1).values
    lo, hi = srt[:, k], srt[:, min(k + 1, a.shape[1] - 1)]
    d = hi - lo
    q = lo + torch.tensor(w, dtype=torch.float32) * d
    return torch.maximum(q, torch.ones_like(q))


def _selection_inputs(geom):
    B, C, HW = geom[:3]
    g = torch.Generator().manual_seed(11 + HW)
    base = torch.randn(B, HW, C, generator=g) * 1.5
    pm = (torch.randint(0, 4, (B, HW, C), generator=g).float() + 0.5) * (torch.randint(0, 2, (B, HW, C), generator=g) * 2 - 1)
    pm[:, ::3] = 0.0                                                  # +-{0.5, 1.5, 2.5, 3.5}, a third of the pixels +-0
    pm[:, 1::6] = -0.0
    return {"randn": base,
            "quantised": (base * 4).round() / 4,                      # multiples of 0.25: ties, also across k / k + 1
            "plus_minus": pm,
            "below_one": base / (base.abs().max() * 1.0001)}          # the floor: s == 1 exactly


@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_selection_is_exact_bit_for_bit(dev, geom):
    """objective pred_x0: x0 = the network output exactly, so s is the float32 restatement's bits"""
    from lgm_hip import sampler
    B, C, HW = geom[:3]
    for name, vals in _selection_inputs(geom).items():
        xin, v = _buffers(5, geom, vals)
        xd, vd = xin.to(dev), v.to(dev)
        for p in PERCENTILES:
            k, w = sampler.dyn_rank(C * HW, p)
            got = _dyn(dev, geom, xd, vd, OBJ["pred_x0"], None, p)
            want = _restated(vals.reshape(B, -1).abs(), k, w)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, p, got, want)
            assert (got >= 1).all()
            if name == "below_one":
                assert (got == 1).all()
            if name == "randn" and p >= 0.95:
                assert (got > 1).all(), "the threshold acts"
        if name == "quantised":                                       # the k-th and (k+1)-th smallest really tie somewhere
            srt = vals.reshape(B, -1).abs().sort(dim=1).values
            k = sampler.dyn_rank(C * HW, 0.5)[0]
            assert (srt[:, k] == srt[:, k + 1]).any() or HW < 64


@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_every_objective_against_float64(dev, heads, geom):
    """|s - s64| <= max_i(4 u m0_i) + 3 u s64: an order statistic is 1-Lipschitz in the sup norm, every x0 carries three
    roundings inside 4 u m0 (m0 = |p x| + |q v|, |v| for pred_x0), and the interpolation's difference, product and sum round
    once each, relative to partial results that q <= s64 bounds."""
    from lgm_hip import sampler
    B, C, HW, pitch, x_off, sc_off = geom
    for objective in (0, 1, 2):
        for t in (999, 500, 0):
            A, Bv, R, Rm1 = heads["dpm"][t][:4]
            xin, v = _buffers(100 * objective + t, geom)
            x64, v64 = xin[..., x_off:x_off + C].double(), v[..., :C].double()
            pc, qc = (R, Rm1) if objective == 0 else (A, -Bv)
            if objective == 1:
                x0, m0 = v64, v64.abs()
            else:
                x0, m0 = pc * x64 - qc * v64, (pc * x64).abs() + (qc * v64).abs()
            srt = x0.reshape(B, -1).abs().sort(dim=1).values
            xd, vd = xin.to(dev), v.to(dev)
            for p in (0.5, 0.995):
                k, w = sampler.dyn_rank(C * HW, p)
                lo, hi = srt[:, k], srt[:, min(k + 1, C * HW - 1)]
                s64 = (lo + w * (hi - lo)).clamp(min=1.0)
                got = _dyn(dev, geom, xd, vd, objective, (A, Bv, R, Rm1), p).double()
                bound = 4 * U * m0.reshape(B, -1).max(dim=1).values + 3 * U * s64
                assert float(((got - s64).abs() - bound).max()) <= 0, (objective, t, p, got, s64)


@pytest.mark.parametrize("geom", GEOMS[:3], ids=GIDS[:3])
def test_table_form_equals_by_value_form(dev, heads, geom):
    xin, v = _buffers(9, geom)
    xd, vd = xin.to(dev), v.to(dev)
    table = torch.zeros(4, 8)
    for i, t in enumerate((999, 0, 500)):
        table[i] = torch.tensor(heads["dpm"][t])
    td = table.to(dev)
    for at, t in ((0, 999), (2, 500)):
        counter = torch.full((1,), at, dtype=torch.int32, device=dev)
        for objective in (0, 2):
            want = _dyn(dev, geom, xd, vd, objective, heads["dpm"][t], 0.95)
            got = _dyn(dev, geom, xd, vd, objective, None, 0.95, td, counter)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and int(counter.item()) == at
    assert not torch.equal(_dyn(dev, geom, xd, vd, 2, heads["dpm"][999], 0.95), _dyn(dev, geom, xd, vd, 2, heads["dpm"][500], 0.95))


# ----------------------------------------------------------------------------------------------------------------------
# the update kernels with a threshold buffer.  Bounds, with s the kernel's own float32 threshold and m0 as above:
#   x0     |x0 - clamp(x0_64, -s, s) / s| <= 4 u m0 / s + u: the three roundings of the unclipped x0 scaled by 1 / s (the clamp
#          moves nothing further away), one for a quotient of magnitude <= 1;
#   next x 8 u M as in tests/test_hip_dpmpp.py / tests/test_hip_selfcond.py with m0x = m0 / s + 1 in the place of m0:
#          M = |K_x x| + |K_0| m0x + |K_1 hist| + |K_n noise| for the solver step, C_0 m0x + |C_1 x| + C_2 m_eps + |C_3 noise|
#          for the ancestral / DDIM step, m_eps = |v| where the noise is the raw network output, else ((|R x| + |x0| + m0x) /
#          Rm1 + |eps|).
# ----------------------------------------------------------------------------------------------------------------------
def _x0_64(geom, xin, v, head, objective, s):
    """float64 from the float32 head -> (thresholded x0, unclipped magnitude bound m0), s [B] the kernel's thresholds"""
    B, C, HW, pitch, x_off, sc_off = geom
    A, Bv, R, Rm1 = head[:4]
    x64, v64 = xin[..., x_off:x_off + C].double(), v[..., :C].double()
    pc, qc = (R, Rm1) if objective == 0 else (A, -Bv)
    if objective == 1:
        x0, m0 = v64.clone(), v64.abs()
    else:
        x0, m0 = pc * x64 - qc * v64, (pc * x64).abs() + (qc * v64).abs()
    sv = s.double().view(B, 1, 1)
    return torch.maximum(torch.minimum(x0, sv), -sv) / sv, m0, sv


def _pads(geom):
    B, C, HW, pitch, x_off, sc_off = geom
    pad = torch.ones(pitch, dtype=torch.bool)
    pad[x_off:x_off + C] = False
    if sc_off >= 0:
        pad[sc_off:sc_off + C] = False
    return pad


def _dpm_thresh(geom, xin, xout, v, nz, hist, objective, row, thresh, table=None, counter=None, advance=0):
    from lgm_hip import ops
    B, C, HW, pitch, x_off, sc_off = geom
    row = (0.0,) * 8 if row is None else row
    ops.lib().lgm_dpm_step_thresh(xin.data_ptr(), xout.data_ptr(), pitch, x_off, sc_off, v.data_ptr(), v.shape[-1],
                                  None if nz is None else nz.data_ptr(), hist.data_ptr(), B, C, HW, objective, *row,
                                  None if table is None else table.data_ptr(),
                                  None if counter is None else counter.data_ptr(), advance, thresh.data_ptr(), ops.stream())
    assert ops.lib()._dll.lgm_last_kernel().decode() == "dpm_step_kernel"


def _sample_thresh(geom, xin, xout, v, nz, x0_out, objective, rederive, row, thresh, table=None, counter=None, advance=0):
    from lgm_hip import ops
    B, C, HW, pitch, x_off, sc_off = geom
    row = (0.0,) * 8 if row is None else row
    ops.lib().lgm_sample_step_thresh(xin.data_ptr(), xout.data_ptr(), pitch, x_off, sc_off, v.data_ptr(), v.shape[-1],
                                     None if nz is None else nz.data_ptr(), None if x0_out is None else x0_out.data_ptr(),
                                     B, C, HW, objective, 1 if rederive else 0, *row,
                                     None if table is None else table.data_ptr(),
                                     None if counter is None else counter.data_ptr(), advance, thresh.data_ptr(),
                                     ops.stream())
    assert ops.lib()._dll.lgm_last_kernel().decode() == "sample_step_slice_kernel"


@pytest.mark.parametrize("geom", GEOMS[:3], ids=GIDS[:3])
def test_dpm_step_with_thresholds_against_float64(dev, heads, geom):
    B, C, HW, pitch, x_off, sc_off = geom
    Cp = _r4(C)
    g = torch.Generator().manual_seed(21)
    nz = torch.randn(B, C, HW, generator=g)
    hist0 = torch.full((B, HW, Cp), NAN)
    hist0[..., :C] = torch.rand(B, HW, C, generator=g) * 2 - 1
    for objective in (0, 1, 2):
        for t in (999, 500, 0):
            row = heads["dpm"][t]
            xin, v = _buffers(1000 * objective + t, geom)
            xd, vd, nd = xin.to(dev), v.to(dev), nz.to(dev)
            s = _dyn(dev, geom, xd, vd, objective, row, 0.95)
            sd = s.to(dev)
            out, hd = torch.full_like(xd, NAN), hist0.to(dev)
            _dpm_thresh(geom, xd, out, vd, nd, hd, objective, row, sd)
            out, hd = out.cpu(), hd.cpu()
            x0, m0, sv = _x0_64(geom, xin, v, row, objective, s)
            what = (objective, t)
            assert float(((hd[..., :C].double() - x0).abs() - (4 * U * m0 / sv + U)).max()) <= 0, what
            assert float(hd[..., :C].abs().max()) <= 1.0, what
            assert not hd[..., C:].any(), "pad lanes of the history come out zero"
            Kx, K0, K1, Kn = row[4:]
            x64, h64 = xin[..., x_off:x_off + C].double(), hist0[..., :C].double()
            n64 = nz.permute(0, 2, 1).double()
            o = Kx * x64 + K0 * x0 + (K1 * h64 if K1 != 0.0 else 0.0) + Kn * n64
            M = (Kx * x64).abs() + abs(K0) * (m0 / sv + 1) + (K1 * h64).abs() * (K1 != 0.0) + (Kn * n64).abs()
            assert float(((out[..., x_off:x_off + C].double() - o).abs() - 8 * U * M).max()) <= 0, what
            pad = _pads(geom)
            if sc_off >= 0:
                assert torch.equal(out[..., sc_off:sc_off + C], hd[..., :C]), "the x0 handed to the next step"
            assert pad.any() and not out[..., pad].any(), "pad lanes of the next input buffer come out zero"
            assert torch.equal(xd.cpu()[..., x_off:x_off + C], xin[..., x_off:x_off + C]), "out of place: input read only"
            # in place == out of place
            inp, hi = xin.to(dev), hist0.to(dev)
            _dpm_thresh(geom, inp, inp, vd, nd, hi, objective, row, sd)
            assert torch.equal(inp.cpu(), out) and torch.equal(hi.cpu(), hd), what
            # the table + counter form == the by-value form; advance appends counter += 1
            table = torch.zeros(3, 8)
            table[1] = torch.tensor(row)
            counter = torch.ones(1, dtype=torch.int32, device=dev)
            inp, hi = xin.to(dev), hist0.to(dev)
            _dpm_thresh(geom, inp, inp, vd, nd, hi, objective, None, sd, table.to(dev), counter, 1)
            assert torch.equal(inp.cpu(), out) and torch.equal(hi.cpu(), hd) and int(counter.item()) == 2, what
            # thresholds of one: the static clamp's bits (the static entry point reads no NaN lane either)
            one = torch.ones(B, device=dev)
            a, ha = torch.full_like(xd, NAN), hist0.to(dev)
            _dpm_thresh(geom, xd, a, vd, nd, ha, objective, row, one)
            b, hb = torch.full_like(xd, NAN), hist0.to(dev)
            from lgm_hip import ops
            ops.lib().lgm_dpm_step(xd.data_ptr(), b.data_ptr(), pitch, x_off, sc_off, vd.data_ptr(), vd.shape[-1], nd.data_ptr(),
                                   hb.data_ptr(), B, C, HW, objective, row[0], row[1], 1, *row[2:], ops.stream())
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ha.view(torch.int32),
                                                                                           hb.view(torch.int32)), what


@pytest.mark.parametrize("geom", GEOMS[:3], ids=GIDS[:3])
def test_sample_step_with_thresholds_against_float64(dev, heads, geom):
    B, C, HW, pitch, x_off, sc_off = geom
    g = torch.Generator().manual_seed(22)
    nz = torch.randn(B, C, HW, generator=g)
    for objective in (0, 1, 2):
        for t in (999, 500, 0):
            for rederive in (False, True):
                row = heads["ddim"][t]
                A, Bv, R, Rm1, C0, C1, C2, C3 = row
                xin, v = _buffers(2000 * objective + t, geom)
                xd, vd, nd = xin.to(dev), v.to(dev), nz.to(dev)
                s = _dyn(dev, geom, xd, vd, objective, row, 0.95)
                sd = s.to(dev)
                out = torch.full_like(xd, NAN)
                x0_out = torch.full_like(xd, NAN) if sc_off < 0 else None
                _sample_thresh(geom, xd, out, vd, nd, x0_out, objective, rederive, row, sd)
                outc = out.cpu()
                x0, m0, sv = _x0_64(geom, xin, v, row, objective, s)
                m0x = m0 / sv + 1
                got_x0 = (outc[..., sc_off:sc_off + C] if sc_off >= 0 else x0_out.cpu()[..., :C])
                what = (objective, t, rederive)
                assert float(((got_x0.double() - x0).abs() - (4 * U * m0 / sv + U)).max()) <= 0, what
                assert float(got_x0.abs().max()) <= 1.0, what
                if x0_out is not None:
                    assert not x0_out.cpu()[..., C:].any(), "pad lanes of the returned x0 come out zero"
                x64, v64, n64 = xin[..., x_off:x_off + C].double(), v[..., :C].double(), nz.permute(0, 2, 1).double()
                if objective == 0 and not rederive:
                    eps, m_eps = v64, v64.abs()
                else:                                                  # the noise comes from the THRESHOLDED x0
                    eps = (R * x64 - x0) / Rm1
                    m_eps = ((R * x64).abs() + x0.abs() + m0x) / Rm1 + eps.abs()
                o = C0 * x0 + C1 * x64 + C2 * eps + C3 * n64
                M = abs(C0) * m0x + (C1 * x64).abs() + abs(C2) * m_eps + (C3 * n64).abs()
                assert float(((outc[..., x_off:x_off + C].double() - o).abs() - 8 * U * M).max()) <= 0, what
                if objective == 0 and rederive and t == 500:
                    # the bound tells the noise re-derived from the thresholded x0 from the raw network output and from the
                    # noise of a statically clamped x0
                    eps_static = (R * x64 - (R * x64 - Rm1 * v64).clamp(-1.0, 1.0)) / Rm1
                    assert float((C2 * (eps_static - eps)).abs().max()) > 1e-3
                    assert float((C2 * (v64 - eps)).abs().max()) > 1e-3
                pad = _pads(geom)
                assert pad.any() and not outc[..., pad].any(), "pad lanes of the next input buffer come out zero"
                # in place == out of place
                inp = xin.to(dev)
                x0_b = torch.full_like(xd, NAN) if sc_off < 0 else None
                _sample_thresh(geom, inp, inp, vd, nd, x0_b, objective, rederive, row, sd)
                assert torch.equal(inp.cpu(), outc), what
                if x0_b is not None:
                    assert torch.equal(x0_b, x0_out)
                # the table + counter form == the by-value form; advance appends counter += 1
                table = torch.zeros(3, 8)
                table[2] = torch.tensor(row)
                counter = torch.full((1,), 2, dtype=torch.int32, device=dev)
                inp = xin.to(dev)
                _sample_thresh(geom, inp, inp, vd, nd, None, objective, rederive, None, sd, table.to(dev), counter, 1)
                assert torch.equal(inp.cpu(), outc) and int(counter.item()) == 3, what
                # thresholds of one: the static clamp's bits
                from lgm_hip import ops
                one = torch.ones(B, device=dev)
                a, b = torch.full_like(xd, NAN), torch.full_like(xd, NAN)
                _sample_thresh(geom, xd, a, vd, nd, None, objective, rederive, row, one)
                ops.lib().lgm_sample_step_slice(xd.data_ptr(), b.data_ptr(), pitch, x_off, sc_off, vd.data_ptr(), vd.shape[-1],
                                                nd.data_ptr(), B, C, HW, objective, A, Bv, 1, 1 if rederive else 0, R, Rm1, C0,
                                                C1, C2, C3, ops.stream())
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def test_model_predictions_with_thresholds(dev):
    """the composition behind ``model_predictions(clip_x_start=True)``: unclipped predictions, lgm_dyn_thresh over the dense
    x_start as a one-channel pred_x0 problem, predictions with the thresholds - against float64, and thresholds of one
    against the static clip bit for bit"""
    from lgm_hip import ops, sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000).to(dev)
    B, per = 3, 3 * 25
    g = torch.Generator().manual_seed(31)
    x, v = torch.randn(B, per, generator=g) * 1.5, torch.randn(B, per, generator=g)
    t = torch.tensor([999, 500, 0])
    xd, vd, td = x.to(dev), v.to(dev), t.to(dev)
    names = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
             "sqrt_recipm1_alphas_cumprod")
    tabs = [getattr(gd, n).data_ptr() for n in names]
    A, S, R, Rm1 = (getattr(gd, n).cpu()[t].double()[:, None] for n in names)
    L = ops.lib()
    k, w = sampler.dyn_rank(per, 0.95)
    for objective in (0, 1, 2):
        for rederive in (0, 1):
            pn, xs = torch.empty_like(xd), torch.empty_like(xd)
            L.lgm_model_predictions_obj(xd.data_ptr(), vd.data_ptr(), td.data_ptr(), *tabs, objective, 0, rederive, pn.data_ptr(),
                                        xs.data_ptr(), B, per, 1000, ops.stream())
            s = torch.empty(B, device=dev)
            L.lgm_dyn_thresh(xd.data_ptr(), 1, 0, xs.data_ptr(), 1, B, 1, per, 1, 0.0, 0.0, 0.0, 0.0, None, None, k, w,
                             s.data_ptr(), ops.stream())
            assert torch.equal(s.cpu(), _restated(xs.cpu().abs(), k, w)), "x0 = the unclipped x_start, bit for bit"
            L.lgm_model_predictions_thresh(xd.data_ptr(), vd.data_ptr(), td.data_ptr(), *tabs, objective, rederive,
                                           pn.data_ptr(), xs.data_ptr(), B, per, 1000, s.data_ptr(), ops.stream())
            x64, v64, sv = x.double(), v.double(), s.cpu().double()[:, None]
            pc, qc = (R, Rm1) if objective == 0 else (A, S)
            x0, m0 = (v64, v64.abs()) if objective == 1 else (pc * x64 - qc * v64, (pc * x64).abs() + (qc * v64).abs())
            x0 = torch.maximum(torch.minimum(x0, sv), -sv) / sv
            assert float(((xs.cpu().double() - x0).abs() - (4 * U * m0 / sv + U)).max()) <= 0
            assert float(xs.abs().max()) <= 1.0
            if objective == 0 and not rederive:
                assert torch.equal(pn, vd)
            else:
                eps = (R * x64 - x0) / Rm1
                m = ((R * x64).abs() + x0.abs() + m0 / sv + 1) / Rm1 + eps.abs()
                assert float(((pn.cpu().double() - eps).abs() - 8 * U * m).max()) <= 0
            a_pn, a_xs, b_pn, b_xs = (torch.empty_like(xd) for _ in range(4))
            one = torch.ones(B, device=dev)
            L.lgm_model_predictions_thresh(xd.data_ptr(), vd.data_ptr(), td.data_ptr(), *tabs, objective, rederive,
                                           a_pn.data_ptr(), a_xs.data_ptr(), B, per, 1000, one.data_ptr(), ops.stream())
            L.lgm_model_predictions_obj(xd.data_ptr(), vd.data_ptr(), td.data_ptr(), *tabs, objective, 1, rederive,
                                        b_pn.data_ptr(), b_xs.data_ptr(), B, per, 1000, ops.stream())
            assert torch.equal(a_pn.view(torch.int32), b_pn.view(torch.int32)) and torch.equal(a_xs.view(torch.int32),
                                                                                                b_xs.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# chains against the reference fixture; graph replay against eager launches
# ----------------------------------------------------------------------------------------------------------------------
KINDS = {"ode2m": dict(kind="dpm"), "ode2m_p95": dict(kind="dpm", p="p_low"), "sde2m": dict(kind="dpm", stochastic=True),
         "ddim0": dict(kind="ddim", eta=0.0), "ddim1": dict(kind="ddim", eta=1.0), "ancestral": dict(kind="ancestral"),
         "selfcond": dict(kind="dpm", net="selfcond"), "guided": dict(kind="dpm", net="guided")}
CHAINS = [("pred_v", "ode2m"), ("pred_noise", "ode2m"), ("pred_v", "ode2m_p95"), ("pred_v", "sde2m"), ("pred_v", "ddim0"),
          ("pred_noise", "ddim0"), ("pred_v", "ddim1"), ("pred_noise", "ddim1"), ("pred_v", "ancestral"),
          ("pred_v", "selfcond"), ("pred_v", "guided")]


@pytest.fixture(scope="module")
def nets(fx, dev):
    """the three networks of the fixture, built once"""
    from models.generative.diffusion.ddpm import Unet
    from oracle import diffusion as OD
    P = OD.unet_init(dim=int(fx["dim"]), channels=3, seed=int(fx["seed"]))
    out = {}
    for kind, kw, extra in (("plain", {}, {}),
                            ("selfcond", dict(self_condition=True), {"init_conv.weight": fx["sc:init_conv.weight"]}),
                            ("guided", dict(num_classes=int(fx["K"])), {"label_emb.weight": fx["label_emb.weight"]})):
        net = Unet(dim=int(fx["dim"]), channels=3, **kw)
        net.load_state_dict(dict(P, **{k: torch.as_tensor(v) for k, v in extra.items()}), strict=True)
        out[kind] = net
    return out


def _arbiter(parity, what, hip, ref, exact=None):
    """1e-4 against the reference's fp32 result; with ``exact`` (the fixture's float64 evaluation) a miss is decided by
    float64 - HIP no further from it than twice the reference itself.  Both distances to float64 go on record either way."""
    e = rel(hip, ref)
    if exact is not None:
        parity.record(what + " [distances to float64]", hip_vs_ref=e, ref_vs_fp64=rel(ref, exact), hip_vs_fp64=rel(hip, exact))
    if e < RTOL or exact is None:
        return parity(what, e, RTOL)
    d_ref, d_hip = rel(ref, exact), rel(hip, exact)
    print(f"[parity] {what}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, hip {d_hip:.3e}")
    assert d_hip <= 2 * d_ref, (what, e, d_hip, d_ref)


def _diffusion(fx, net, objective, name, dev):
    """the thresholding diffusion of a fixture chain -> (diffusion, run(init, noises, classes, scale), first_step(chain, nz0))"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion
    spec = KINDS[name]
    S, steps = int(fx["S"]), int(fx["steps"])
    kw = dict(img_size=S, objective=objective, dynamic_thresholding=True,
              dynamic_thresholding_percentile=float(fx[spec.get("p", "p")]))
    if spec["kind"] == "dpm":
        gd = GaussianDiffusion(net, timesteps=int(fx["T"]), sampling_timesteps=steps, sampler="dpm++",
                               dpm_stochastic=spec.get("stochastic", False), **kw).to(dev)
        loop = sampler.dpm_solver_sample

        def first(chain, nz0):
            pairs = gd.dpm_time_pairs()
            sampler.dpm_step(chain, pairs[0][0], nz0, sampler.dpm_coeffs(gd, pairs, gd.dpm_order, gd.dpm_stochastic)[0])
    elif spec["kind"] == "ddim":
        gd = GaussianDiffusion(net, timesteps=int(fx["T"]), sampling_timesteps=steps, ddim_sampling_eta=spec["eta"], **kw).to(dev)
        loop = sampler.ddim_sample

        def first(chain, nz0):
            t, t_next = gd.ddim_time_pairs()[0]
            sampler.ddim_step(chain, t, t_next, nz0, gd.ddim_sampling_eta)
    else:
        gd = GaussianDiffusion(net, timesteps=int(fx["ancestral_T"]), **kw).to(dev)
        loop = sampler.p_sample_loop

        def first(chain, nz0):
            sampler.p_sample_step(chain, gd.num_timesteps - 1, nz0)
    return gd, loop, first


def _thresh_keys(net):
    from lgm_hip import sampler
    return [k for k, e in sampler._GRAPHS.get(net, {}).items() if k[0] == "dynthresh" and isinstance(e, sampler._GraphedChain)]


@pytest.mark.parametrize("objective,name", CHAINS, ids=[f"{o}-{k}" for o, k in CHAINS])
def test_chains_match_reference_fixture_and_graph_replay_equals_eager(fx, nets, dev, parity, monkeypatch, objective, name):
    from lgm_hip import sampler
    from oracle import diffusion as OD
    spec = KINDS[name]
    net = nets[spec.get("net", "plain")]
    gd, loop, first = _diffusion(fx, net, objective, name, dev)
    net.prepare_hip(dev)
    B, S = int(fx["B"]), int(fx["S"])
    steps = int(fx["ancestral_T"]) if spec["kind"] == "ancestral" else int(fx["steps"])
    shape = (B, 3, S, S)
    init, nz = OD.draw_loop_noise(int(fx[f"{name}_seed"]), shape, steps - 1)
    guided = spec.get("net") == "guided"
    y = torch.as_tensor(fx["classes"]).to(dev) if guided else None
    scale = float(fx["cond_scale"]) if guided else 1.0

    def run():
        return loop(gd, shape, init_noise=init.to(dev), noises=[x.to(dev) for x in nz] + [None], classes=y,
                    cond_scale=scale).clone()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = run()
    # the thresholded step's own cache key: the static step's key behind ("dynthresh", percentile)
    kind = spec["kind"]
    key = (shape, {"dpm": spec.get("stochastic", False), "ddim": spec.get("eta", 0.0) != 0.0, "ancestral": True}[kind])
    if objective != "pred_v":
        key += (objective, kind == "ddim")
    if guided:
        key += ("guided",)
    if kind == "dpm":
        key = ("dpm++", objective) + key
    key = ("dynthresh", gd.dynamic_thresholding_percentile) + key
    assert key in _thresh_keys(net), f"graph capture of the thresholded step did not happen: {_thresh_keys(net)}"
    again = run()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run()
    what = f"{objective}: thresholded chain, {name}"
    assert torch.isfinite(graph).all() and float(graph.std()) > 0
    assert torch.equal(graph, eager), f"{what}: graph replay differs from eager launches"
    assert torch.equal(graph, again), f"{what}: the second chain on one captured step differs from the first"
    _arbiter(parity, f"{what}, final image", graph, fx[f"{objective}:{name}"], unpack64(fx, f"{objective}:{name}"))
    # the first step as the eager chain takes it: the thresholded x0 it hands on and the thresholds themselves
    chain = sampler._Chain(gd, shape, init.to(dev), None, y, scale)
    first(chain, nz[0].to(dev))
    x0 = chain.x0[..., :3].permute(0, 3, 1, 2)
    _arbiter(parity, f"{what}, x0 of the first step", x0, fx[f"{objective}:{name}:x0_first"],
             unpack64(fx, f"{objective}:{name}:x0_first"))
    assert float(x0.abs().max()) <= 1.0
    s_ref = fx[f"{objective}:{name}:s"][0]
    parity(f"{what}, thresholds of the first step", rel(chain.thresh, s_ref), RTOL)
    assert (chain.thresh >= 1).all()


def test_two_percentiles_on_one_network_each_match_their_fixture(fx, nets, dev, parity, monkeypatch):
    """p = 0.995 and p = 0.95 on the same network: the rank is baked into the captured launch, the percentile is in the key"""
    from oracle import diffusion as OD
    net = nets["plain"]
    net.prepare_hip(dev)
    shape = (int(fx["B"]), 3, int(fx["S"]), int(fx["S"]))
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    # both chains from the SAME draws (ode2m's), so that nothing but the percentile tells them apart ...
    init, _ = OD.draw_loop_noise(int(fx["ode2m_seed"]), shape, 9)
    hi, loop, _ = _diffusion(fx, net, "pred_v", "ode2m", dev)
    lo, _, _ = _diffusion(fx, net, "pred_v", "ode2m_p95", dev)
    a = loop(hi, shape, init_noise=init.to(dev)).clone()
    b = loop(lo, shape, init_noise=init.to(dev)).clone()
    a2 = loop(hi, shape, init_noise=init.to(dev)).clone()
    assert torch.equal(a, a2) and not torch.equal(a, b), "two percentiles share baked constants"
    keys = _thresh_keys(net)
    assert {k[1] for k in keys} >= {0.95, 0.995}
    parity("pred_v: p = 0.995 beside p = 0.95 on one network", rel(a, fx["pred_v:ode2m"]), RTOL)
    # ... and the p = 0.95 chain from its own draws against its own fixture, after the other percentile ran
    init95, _ = OD.draw_loop_noise(int(fx["ode2m_p95_seed"]), shape, 9)
    c = loop(lo, shape, init_noise=init95.to(dev))
    parity("pred_v: p = 0.95 beside p = 0.995 on one network", rel(c, fx["pred_v:ode2m_p95"]), RTOL)


def test_static_clip_chains_beside_thresholded_ones_keep_their_bits(fx, dev, monkeypatch):
    """a DDIM chain and a dpm++ chain with the static clamp, before and after thresholded chains on the same network: the same
    bits, under their old cache keys"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    net = Unet(dim=16, channels=3)
    net.load_state_dict(OD.unet_init(dim=16, channels=3, seed=int(fx["seed"])), strict=True)
    mk = lambda **kw: GaussianDiffusion(net, img_size=16, sampling_timesteps=6, **kw).to(dev)  # noqa: E731
    ddim, dpm = mk(), mk(sampler="dpm++")
    ddim_t, dpm_t = mk(dynamic_thresholding=True), mk(sampler="dpm++", dynamic_thresholding=True)
    assert ddim_t.is_ddim_sampling and not ddim.dynamic_thresholding
    net.prepare_hip(dev)
    shape = (2, 3, 16, 16)
    init = torch.randn(shape, generator=torch.Generator().manual_seed(6)).to(dev)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    before = (sampler.ddim_sample(ddim, shape, init_noise=init).clone(), sampler.dpm_solver_sample(dpm, shape, init_noise=init).clone())
    old_keys = set(sampler._GRAPHS[net])
    assert len(old_keys) == 2 and not _thresh_keys(net)
    assert old_keys == {((2, 3, 16, 16), False), ("dpm++", "pred_v", (2, 3, 16, 16), False)}, "the existing keys are unchanged"
    thr = (sampler.ddim_sample(ddim_t, shape, init_noise=init).clone(), sampler.dpm_solver_sample(dpm_t, shape, init_noise=init).clone())
    assert len(_thresh_keys(net)) == 2 and len(sampler._GRAPHS[net]) == 4
    after = (sampler.ddim_sample(ddim, shape, init_noise=init).clone(), sampler.dpm_solver_sample(dpm, shape, init_noise=init).clone())
    for a, b, c in zip(before, after, thr):
        assert torch.equal(a, b), "a static-clip chain changed its bits beside a thresholded one"
        assert torch.isfinite(c).all() and not torch.equal(a, c)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    assert torch.equal(sampler.ddim_sample(ddim, shape, init_noise=init), before[0])
    assert torch.equal(sampler.dpm_solver_sample(dpm, shape, init_noise=init), before[1])
    assert torch.equal(sampler.ddim_sample(ddim_t, shape, init_noise=init), thr[0])


def test_p_sample_equals_p_mean_variance_and_model_predictions(nets, dev):
    """the x_start of one thresholded ancestral step (thresholds inside the chain's kernels, NHWC slices) is p_mean_variance's
    (the three-launch composition over dense NCHW tensors), bit for bit; ``clip_x_start=False`` stays unclipped"""
    from models.generative.diffusion.ddpm import GaussianDiffusion
    for kind in ("plain", "selfcond"):
        net = nets[kind]
        gd = GaussianDiffusion(net, img_size=16, timesteps=1000, dynamic_thresholding=True).to(dev)
        static = GaussianDiffusion(net, img_size=16, timesteps=1000).to(dev)
        net.prepare_hip(dev)
        g = torch.Generator().manual_seed(8)
        x = (torch.randn(3, 3, 16, 16, generator=g) * 1.2).to(dev)
        sc = (torch.rand(3, 3, 16, 16, generator=g) * 2 - 1).to(dev) if kind == "selfcond" else None
        for t in (999, 400, 0):
            tb = torch.full((3,), t, device=dev, dtype=torch.long)
            img, x0 = gd.p_sample(x, t, sc, noise=torch.zeros_like(x))
            mean, _, _, x0_pmv = gd.p_mean_variance(x, tb, sc)
            assert torch.equal(x0.view(torch.int32), x0_pmv.view(torch.int32)), (kind, t)
            assert float(x0.abs().max()) <= 1.0
            pred = gd.model_predictions(x, tb, sc, clip_x_start=True, rederive_pred_noise=True)
            assert torch.equal(pred.pred_x_start, x0_pmv)
            raw = gd.model_predictions(x, tb, sc, clip_x_start=False).pred_x_start
            assert torch.equal(raw, static.model_predictions(x, tb, sc, clip_x_start=False).pred_x_start)
            s = torch.quantile(raw.flatten(1).abs().double(), 0.995, dim=1).clamp(min=1).view(-1, 1, 1, 1)
            assert rel(x0, torch.maximum(torch.minimum(raw.double(), s), -s) / s) < 1e-5
            if float(s.max()) > 1:
                assert not torch.equal(x0, static.p_sample(x, t, sc, noise=torch.zeros_like(x))[1])
            assert torch.equal(gd.p_mean_variance(x, tb, sc, clip_denoised=False)[3], raw)


def test_sample_and_interpolate_dispatch_under_thresholding(nets, dev):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    net = nets["plain"]
    net.prepare_hip(dev)
    out = {}
    for name, kw in (("ancestral", dict(timesteps=8)), ("ddim", dict(timesteps=1000, sampling_timesteps=4)),
                     ("dpm++", dict(timesteps=1000, sampling_timesteps=4, sampler="dpm++"))):
        for dyn in (False, True):
            gd = GaussianDiffusion(net, img_size=16, dynamic_thresholding=dyn, **kw).to(dev)
            torch.manual_seed(4)
            a = gd.sample(batch_size=2)
            assert a.shape == (2, 3, 16, 16) and torch.isfinite(a).all() and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
            torch.manual_seed(4)
            frames = gd.sample(batch_size=2, return_all_timesteps=True)
            assert torch.equal(frames[:, -1], a), "the last frame of the eager chain is the graph-replayed image"
            out[name, dyn] = a
        assert not torch.equal(out[name, False], out[name, True]), name
    gd = GaussianDiffusion(net, img_size=16, timesteps=8, dynamic_thresholding=True).to(dev)
    g = torch.Generator().manual_seed(2)
    x1, x2 = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev), (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    torch.manual_seed(3)
    mid = gd.interpolate(x1, x2, t=5)
    assert mid.shape == x1.shape and torch.isfinite(mid).all() and float(mid.abs().max()) <= 1.0 + 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# train.py
# ----------------------------------------------------------------------------------------------------------------------
def test_train_entry_runs_the_dynthresh_config(tmp_path):
    """train.py's main() on configs/diffusion/ddpm_cond_dynthresh.json at a reduced size (16 x 16, dim 16, 20 diffusion steps,
    5 solver steps: the step-0 sample is a guided, thresholded 5-step chain of 64 images), three steps, in a child process
    with its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "ddpm_cond_dynthresh.json")))
    args = cfg["model"]["args"]
    assert args["dynamic_thresholding"] is True and args["sampler"] == "dpm++" and args["cond_scale"] == 3.0
    args.update(img_size=16, dim=16, diffusion_timesteps=20, sampling_timesteps=5)
    cfg["dataset"].update(img_size=16, batch_size=8)
    path = tmp_path / "ddpm_cond_dynthresh_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_ddpm_cond_dynthresh"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('LAST_SAMPLES', tuple(m.last_samples.shape), bool(torch.isfinite(m.last_samples).all())); "
            "g = m.ema.ema_model; print('SAMPLER', g.sampler, g.sampling_timesteps, g.dynamic_thresholding, g.cond_scale); "
            "print('TRAIN_LOSS', float(m.logged['train_loss']))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "3", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("LAST_SAMPLES", "TRAIN_LOSS", "SAMPLER"))}
    assert lines["LAST_SAMPLES"] == "LAST_SAMPLES (64, 3, 16, 16) True", lines
    assert lines["SAMPLER"] == "SAMPLER dpm++ 5 True 3.0"
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 3 and sd["hyper_parameters"]["dynamic_thresholding"] is True
