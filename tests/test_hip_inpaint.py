"""GPU: inpainting on the HIP path (``GaussianDiffusion.inpaint``; RePaint, Lugmayr et al. 2022, Algorithm 1, an extension of
the reference): known-region sampling with resampling, the tail of ``inpaint_tail_one`` behind both update kernels.

  * the two entry points against float64 (bound below) at the smallest shapes that can go wrong, all objectives, with and
    without a jump and thresholds; the x0 outputs unblended; pad lanes zero; lanes that must not be read hold NaN;
  * binary masks bit for bit: m = 1 is M_a known + M_n eps_k, m = 0 the plain entry point's output;
  * the table form against the by-value form bit for bit;
  * whole chains against tests/golden/diffusion_inpaint.npz (tools/make_golden_inpaint.py: loops around the REFERENCE's
    network), 1e-4 relative with the float64 arbiter rule of tests/test_hip_dynthresh.py; graph replay bit for bit against
    eager launches under injected draws, also through more than one table segment;
  * plain chains before and after inpainting chains keep their bits; ``GaussianDiffusion.inpaint`` / ``DDPM.inpaint``.

Bound of the tail.  E_s <= 8 u M is the update's own bound (tests/test_hip_dynthresh.py, tests/test_hip_dpmpp.py; for the static
clamp m0x = m0).  Every added product or sum rounds once, u = 2^-24 relative to its result, which the magnitudes of its terms
bound.  With Mk = |M_a known| + |M_n eps_k| and |x_s| <= |x_s64| + E_s:
    known_s  two products and a sum                                            2 u Mk
    1 - m    one sum                                                           u (1 - m)
    y        m known_s (+ u m Mk), (1 - m) x_s (+ u (1 - m) |x_s|), their sum (+ u (m Mk + (1 - m) |x_s|)):
             E_y <= (1 - m) E_s + 4 u m Mk + 3 u (1 - m) |x_s|
    jump     J_x y, J_n eps_j, their sum:   E <= J_x E_y + 2 u (|J_x| (|y64| + E_y) + |J_n eps_j|)
"""
import os

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
    return dict(np.load(os.path.join(golden_dir, "diffusion_inpaint.npz")))


def _r4(n):
    return (n + 3) // 4 * 4


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# the two entry points.  (B, C, HW, pitch, x_off, sc_off): B * HW * pitch = 300 / 600 elements - two / three workgroups of
# 256, the last one partial, and with HW = 25 the mask row (and the sample) changes inside a workgroup.
# ----------------------------------------------------------------------------------------------------------------------
GEOMS = [(3, 3, 25, 4, 0, -1), (3, 3, 25, 8, 3, 0), (3, 1, 25, 4, 0, -1)]
GIDS = ["3x3x25", "selfcond_3x3x25", "3x1x25"]
TIMES = (999, 500, 0)


@pytest.fixture(scope="module")
def rows():
    """per t in TIMES: the DDIM (eta 1) and SDE solver rows of the dynthresh tests, and the inpainting row of a walk over the
    grid [0, 250, 500, 750, 999] - t = 999 lands on 750 without a jump, t = 500 lands on 250 and jumps two levels up to 750,
    t = 0 lands on the clean image (1, 0, 1, 0)"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)
    grid = [(999, 750), (750, 500), (500, 250), (250, 0), (0, -1)]
    sde = sampler.dpm_coeffs(gd, grid, 2, True)
    dpm = {999: sde[0], 500: sde[2], 0: sde[4]}
    ddim = {999: sampler._ddim_coeffs(gd, 999, 750, 1.0), 500: sampler._ddim_coeffs(gd, 500, 250, 1.0),
            0: sampler._ddim_coeffs(gd, 0, -1, 1.0)}
    acp = gd.alphas_cumprod.double().tolist()
    ip = sampler.inpaint_plan(acp, [0, 250, 500, 750, 999], [(4, 3, 3), (2, 1, 3), (0, -1, -1)])
    ip = {t: tuple(float(torch.tensor(c, dtype=torch.float32)) for c in r) for t, r in zip(TIMES, ip)}
    assert ip[999][2:] == (1.0, 0.0) and ip[999][1] != 0.0 and ip[500][3] != 0.0 and ip[500][2] < 1.0 and ip[0] == (1.0, 0.0, 1.0, 0.0)
    assert dpm[500][6] != 0.0 and dpm[500][7] != 0.0 and ddim[500][7] != 0.0
    return {"dpm": dpm, "ddim": ddim, "ip": ip}


def _buffers(seed, geom, soft=True):
    """host operands with NaN wherever the kernels must not read: pad lanes and the self-conditioning slice of the input
    buffer, pad lanes of the network output, of the history and of the known image"""
    B, C, HW, pitch, x_off, sc_off = geom
    g = torch.Generator().manual_seed(seed)
    Cp = _r4(C)
    xin = torch.full((B, HW, pitch), NAN)
    xin[..., x_off:x_off + C] = torch.randn(B, HW, C, generator=g) * 1.5
    v = torch.full((B, HW, Cp), NAN)
    v[..., :C] = torch.randn(B, HW, C, generator=g)
    hist = torch.full((B, HW, Cp), NAN)
    hist[..., :C] = torch.rand(B, HW, C, generator=g) * 2 - 1
    known = torch.full((B, HW, Cp), NAN)
    known[..., :C] = torch.rand(B, HW, C, generator=g) * 2 - 1
    nz, ek, ej = (torch.randn(B, C, HW, generator=g) for _ in range(3))
    mask = torch.rand(B, HW, generator=g) if soft else (torch.rand(B, HW, generator=g) < 0.5).float()
    if soft:
        mask[:, 0], mask[:, 1] = 0.0, 1.0                              # the ends of the range among the soft values
    return dict(xin=xin, v=v, hist=hist, known=known, nz=nz, ek=ek, ej=ej, mask=mask)


def _p(t):
    return None if t is None else t.data_ptr()


def _step(kind, geom, d, xin, xout, aux, objective, rederive, row, thresh=None, ip=None, table=None, counter=None, itable=None,
          advance=0, plain=False):
    """one launch of lgm_{sample,dpm}_step_inpaint on the device operands ``d``; ``aux``: x0_out / hist.  ``ip``: the row of 4
    (None with ``itable``); ``plain``: no inpainting operands at all (the update alone)"""
    from lgm_hip import ops
    B, C, HW, pitch, x_off, sc_off = geom
    row = (0.0,) * 8 if row is None else row
    irow = (0.0,) * 4 if ip is None else ip
    tail = (None, None, None, None, 0.0, 0.0, 0.0, 0.0, None) if plain else (
        _p(d["known"]), _p(d["mask"]), _p(d.get("ek")), _p(d.get("ej")), *irow, _p(itable))
    src = (xin.data_ptr(), xout.data_ptr(), pitch, x_off, sc_off, d["v"].data_ptr(), d["v"].shape[-1], _p(d.get("nz")))
    L = ops.lib()
    if kind == "dpm":
        L.lgm_dpm_step_inpaint(*src, aux.data_ptr(), B, C, HW, objective, *row, _p(table), _p(counter), advance, _p(thresh),
                               *tail, ops.stream())
        assert L._dll.lgm_last_kernel().decode() == "dpm_step_kernel"
    else:
        L.lgm_sample_step_inpaint(*src, _p(aux), B, C, HW, objective, 1 if rederive else 0, *row, _p(table), _p(counter),
                                  advance, _p(thresh), *tail, ops.stream())
        assert L._dll.lgm_last_kernel().decode() == "sample_step_slice_kernel"


def _dyn(dev, geom, xd, vd, objective, head):
    from lgm_hip import ops, sampler
    B, C, HW, pitch, x_off, sc_off = geom
    k, w = sampler.dyn_rank(C * HW, 0.95)
    s = torch.full((B,), NAN, device=dev)
    ops.lib().lgm_dyn_thresh(xd.data_ptr(), pitch, x_off, vd.data_ptr(), vd.shape[-1], B, C, HW, objective, *head[:4], None, None,
                             k, w, s.data_ptr(), ops.stream())
    return s


def _update64(kind, geom, h, objective, rederive, row, s):
    """float64 from the float32 operands -> (x_s, its bound E_s = 8 u M, the clipped x0); s [B] thresholds or None"""
    B, C, HW, pitch, x_off, sc_off = geom
    A, Bv, R, Rm1, W0, W1, W2, W3 = row
    x64, v64 = h["xin"][..., x_off:x_off + C].double(), h["v"][..., :C].double()
    n64 = h["nz"].permute(0, 2, 1).double()
    pc, qc = (R, Rm1) if objective == 0 else (A, -Bv)
    if objective == 1:
        x0, m0 = v64.clone(), v64.abs()
    else:
        x0, m0 = pc * x64 - qc * v64, (pc * x64).abs() + (qc * v64).abs()
    if s is None:
        x0, m0x = x0.clamp(-1.0, 1.0), m0
    else:
        sv = s.double().cpu().view(B, 1, 1)
        x0, m0x = torch.maximum(torch.minimum(x0, sv), -sv) / sv, m0 / sv + 1
    if kind == "dpm":
        h64 = h["hist"][..., :C].double()
        o = W0 * x64 + W1 * x0 + (W2 * h64 if W2 != 0.0 else 0.0) + W3 * n64
        M = (W0 * x64).abs() + abs(W1) * m0x + (W2 * h64).abs() * (W2 != 0.0) + (W3 * n64).abs()
    else:
        if objective == 0 and not rederive:
            eps, m_eps = v64, v64.abs()
        else:
            eps = (R * x64 - x0) / Rm1
            m_eps = ((R * x64).abs() + x0.abs() + m0x) / Rm1 + eps.abs()
        o = W0 * x0 + W1 * x64 + W2 * eps + W3 * n64
        M = abs(W0) * m0x + (W1 * x64).abs() + abs(W2) * m_eps + (W3 * n64).abs()
    return o, 8 * U * M, x0


def _tail64(geom, h, o, E_s, irow):
    """the tail in float64 and its bound (module docstring)"""
    B, C, HW, pitch, x_off, sc_off = geom
    Ma, Mn, Jx, Jn = irow
    k64, m = h["known"][..., :C].double(), h["mask"].double()[..., None]
    ek, ej = h["ek"].permute(0, 2, 1).double(), h["ej"].permute(0, 2, 1).double()
    Mk = (Ma * k64).abs() + (Mn * ek).abs()
    y = m * (Ma * k64 + Mn * ek) + (1 - m) * o
    xs_mag = o.abs() + E_s
    E_y = (1 - m) * E_s + 4 * U * m * Mk + 3 * U * (1 - m) * xs_mag
    if (Jx, Jn) == (1.0, 0.0):
        return y, E_y
    return Jx * y + Jn * ej, Jx * E_y + 2 * U * (abs(Jx) * (y.abs() + E_y) + (Jn * ej).abs())


@pytest.mark.parametrize("kind", ["step", "dpm"])
@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_entry_points_against_float64(dev, rows, geom, kind):
    B, C, HW, pitch, x_off, sc_off = geom
    pad = torch.ones(pitch, dtype=torch.bool)
    pad[x_off:x_off + C] = False
    if sc_off >= 0:
        pad[sc_off:sc_off + C] = False
    jumps = 0
    for objective in (0, 1, 2):
        for t in TIMES:
            for rederive in ((False,) if kind == "dpm" else (False, True)):
                for thresholded in (False, True):
                    row, irow = rows["dpm" if kind == "dpm" else "ddim"][t], rows["ip"][t]
                    jumps += irow[2:] != (1.0, 0.0)
                    h = _buffers(1000 * objective + t, geom)
                    d = {k: a.to(dev) for k, a in h.items()}
                    s = _dyn(dev, geom, d["xin"], d["v"], objective, row) if thresholded else None
                    out = torch.full_like(d["xin"], NAN)
                    aux = d["hist"].clone() if kind == "dpm" else (torch.full_like(d["xin"], NAN) if sc_off < 0 else None)
                    # a draw that the row weighs with zero is not read: hand in NaN there
                    dd = dict(d, ek=d["ek"] if irow[1] != 0.0 else torch.full_like(d["ek"], NAN),
                              ej=d["ej"] if irow[3] != 0.0 else torch.full_like(d["ej"], NAN))
                    _step(kind, geom, dd, d["xin"], out, aux, objective, rederive, row, s, irow)
                    outc = out.cpu()
                    what = (kind, objective, t, rederive, thresholded)
                    o, E_s, x0 = _update64(kind, geom, h, objective, rederive, row, s)
                    want, E = _tail64(geom, h, o, E_s, irow)
                    got = outc[..., x_off:x_off + C].double()
                    assert torch.isfinite(got).all(), what
                    assert float(((got - want).abs() - E).max()) <= 0, (what, float(((got - want).abs() / E).max()))
                    # the tail is really there: the plain update is further from the blended result than the bound
                    assert float(((o - want).abs() - E).max()) > 0, what
                    assert pad.any() and not outc[..., pad].any(), "pad lanes of the next input buffer come out zero"
                    # the x0 outputs are the unblended prediction: the bits of the same launch without inpainting operands
                    ref = torch.full_like(d["xin"], NAN)
                    aux_ref = d["hist"].clone() if kind == "dpm" else (torch.full_like(d["xin"], NAN) if sc_off < 0 else None)
                    _step(kind, geom, d, d["xin"], ref, aux_ref, objective, rederive, row, s, plain=True)
                    if aux is not None:
                        assert torch.equal(_bits(aux), _bits(aux_ref)), what
                        assert not aux.cpu()[..., C:].any(), "pad lanes of the x0 output come out zero"
                    if sc_off >= 0:
                        assert torch.equal(_bits(out[..., sc_off:sc_off + C]), _bits(ref[..., sc_off:sc_off + C])), what
                    # in place == out of place
                    inp = d["xin"].clone()
                    aux_b = d["hist"].clone() if kind == "dpm" else (torch.full_like(d["xin"], NAN) if sc_off < 0 else None)
                    _step(kind, geom, dd, inp, inp, aux_b, objective, rederive, row, s, irow)
                    assert torch.equal(_bits(inp), _bits(out)), what
    assert jumps > 0


@pytest.mark.parametrize("kind", ["step", "dpm"])
@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_binary_masks_bit_for_bit(dev, rows, geom, kind):
    """m = 1: M_a known + M_n eps_k in float32, each operation rounded on its own; m = 0: the output of the plain entry point
    (lgm_sample_step_slice / lgm_dpm_step, and the *_thresh ones)"""
    from lgm_hip import ops
    B, C, HW, pitch, x_off, sc_off = geom
    L = ops.lib()
    for objective in (0, 1, 2):
        for t in (999, 0):                                             # rows without a jump: (M_a, M_n, 1, 0) and (1, 0, 1, 0)
            for thresholded in (False, True):
                row, irow = rows["dpm" if kind == "dpm" else "ddim"][t], rows["ip"][t]
                h = _buffers(77 * objective + t, geom, soft=False)
                d = {k: a.to(dev) for k, a in h.items()}
                s = _dyn(dev, geom, d["xin"], d["v"], objective, row) if thresholded else None
                out = torch.full_like(d["xin"], NAN)
                aux = d["hist"].clone() if kind == "dpm" else None
                _step(kind, geom, d, d["xin"], out, aux, objective, True, row, s, irow)
                plain = torch.full_like(d["xin"], NAN)
                src = (d["xin"].data_ptr(), plain.data_ptr(), pitch, x_off, sc_off, d["v"].data_ptr(), d["v"].shape[-1],
                       d["nz"].data_ptr())
                hb = d["hist"].clone()
                if kind == "dpm" and thresholded:
                    L.lgm_dpm_step_thresh(*src, hb.data_ptr(), B, C, HW, objective, *row, None, None, 0, s.data_ptr(), ops.stream())
                elif kind == "dpm":
                    L.lgm_dpm_step(*src, hb.data_ptr(), B, C, HW, objective, row[0], row[1], 1, *row[2:], ops.stream())
                elif thresholded:
                    L.lgm_sample_step_thresh(*src, None, B, C, HW, objective, 1, *row, None, None, 0, s.data_ptr(), ops.stream())
                else:
                    L.lgm_sample_step_slice(*src, B, C, HW, objective, row[0], row[1], 1, 1, *row[2:], ops.stream())
                got, base = out.cpu()[..., x_off:x_off + C], plain.cpu()[..., x_off:x_off + C]
                Ma, Mn = (torch.tensor(c, dtype=torch.float32) for c in irow[:2])
                known_s = Ma * h["known"][..., :C] + Mn * h["ek"].permute(0, 2, 1)
                m = h["mask"].bool()[..., None].expand(B, HW, C)
                what = (kind, objective, t, thresholded)
                assert m.any() and (~m).any()
                assert torch.equal(_bits(got[m]), _bits(known_s[m])), what
                assert torch.equal(_bits(got[~m]), _bits(base[~m])), what
                assert not torch.equal(got[m], base[m])
                if aux is not None:
                    assert torch.equal(_bits(aux), _bits(hb)), "the history is the unblended x0"


@pytest.mark.parametrize("kind", ["step", "dpm"])
@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_table_form_equals_by_value_form(dev, rows, geom, kind):
    """row counter[0] of both tables, in place, advance appends counter += 1; rows at other indices differ"""
    for objective in (0, 2):
        for at, t in ((0, 999), (2, 500), (1, 0)):
            for thresholded in (False, True):
                row, irow = rows["dpm" if kind == "dpm" else "ddim"][t], rows["ip"][t]
                h = _buffers(31 * objective + t, geom)
                d = {k: a.to(dev) for k, a in h.items()}
                s = _dyn(dev, geom, d["xin"], d["v"], objective, row) if thresholded else None
                want = d["xin"].clone()
                aux = d["hist"].clone() if kind == "dpm" else None
                _step(kind, geom, d, want, want, aux, objective, True, row, s, irow)
                table, itable = torch.full((3, 8), 0.25), torch.full((3, 4), 0.75)
                table[at], itable[at] = torch.tensor(row), torch.tensor(irow)
                counter = torch.full((1,), at, dtype=torch.int32, device=dev)
                got = d["xin"].clone()
                aux_t = d["hist"].clone() if kind == "dpm" else None
                _step(kind, geom, d, got, got, aux_t, objective, True, None, s, None, table.to(dev), counter, itable.to(dev), 1)
                what = (kind, objective, t, thresholded)
                assert torch.equal(_bits(got), _bits(want)) and int(counter.item()) == at + 1, what
                if aux is not None:
                    assert torch.equal(_bits(aux_t), _bits(aux)), what


# ----------------------------------------------------------------------------------------------------------------------
# chains against the reference fixture; graph replay against eager launches
# ----------------------------------------------------------------------------------------------------------------------
KINDS = {"ancestral": dict(kind="ancestral"), "ddim0": dict(kind="ddim", eta=0.0), "ddim1": dict(kind="ddim", eta=1.0),
         "ode2m": dict(kind="dpm"), "plain": dict(kind="dpm"), "selfcond": dict(kind="dpm", net="selfcond"),
         "guided": dict(kind="dpm", net="guided", dyn=True)}
CHAINS = [("pred_v", "ancestral"), ("pred_noise", "ancestral"), ("pred_v", "ddim0"), ("pred_noise", "ddim0"), ("pred_v", "ddim1"),
          ("pred_noise", "ddim1"), ("pred_v", "ode2m"), ("pred_v", "plain"), ("pred_v", "selfcond"), ("pred_v", "guided")]


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


def _arbiter(parity, what, hip, ref, exact):
    """1e-4 against the reference's fp32 result; a miss is decided by float64 - HIP no further from it than twice the
    reference itself.  Both distances to float64 go on record either way."""
    e = rel(hip, ref)
    parity.record(what + " [distances to float64]", hip_vs_ref=e, ref_vs_fp64=rel(ref, exact), hip_vs_fp64=rel(hip, exact))
    if e < RTOL:
        return parity(what, e, RTOL)
    d_ref, d_hip = rel(ref, exact), rel(hip, exact)
    print(f"[parity] {what}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, hip {d_hip:.3e}")
    assert d_hip <= 2 * d_ref, (what, e, d_hip, d_ref)


def _diffusion(fx, net, objective, name, dev):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    spec = KINDS[name]
    kw = dict(img_size=int(fx["S"]), objective=objective)
    if spec.get("dyn"):
        kw.update(dynamic_thresholding=True, dynamic_thresholding_percentile=float(fx["p"]))
    if spec["kind"] == "ancestral":
        return GaussianDiffusion(net, timesteps=int(fx["ancestral_T"]), **kw).to(dev)
    if spec["kind"] == "ddim":
        return GaussianDiffusion(net, timesteps=int(fx["T"]), sampling_timesteps=int(fx["steps"]), ddim_sampling_eta=spec["eta"],
                                 **kw).to(dev)
    return GaussianDiffusion(net, timesteps=int(fx["T"]), sampling_timesteps=int(fx["steps"]), sampler="dpm++", **kw).to(dev)


def _inputs(fx, name, gd, dev):
    """-> (plan, known normalised, mask, init, triples) of a fixture chain, on the device"""
    from lgm_hip import sampler
    from oracle import diffusion as OD
    jump = tuple(int(v) for v in fx[f"{name}_jump"])
    plan = sampler._plan_inpaint(gd, *jump)
    shape = (int(fx["B"]), 3, int(fx["S"]), int(fx["S"]))
    init, nz = OD.draw_loop_noise(int(fx[f"{name}_seed"]), shape, 3 * len(plan.times))
    trips = [tuple(nz[3 * i + k].to(dev) for k in range(3)) for i in range(len(plan.times))]
    known = (torch.as_tensor(fx["known"]) * 2 - 1).to(dev)
    return plan, jump, known, torch.as_tensor(fx["mask"]).to(dev), init.to(dev), trips


def _inpaint_keys(net):
    from lgm_hip import sampler
    return [k for k, e in sampler._GRAPHS.get(net, {}).items() if k[0] == "inpaint" and isinstance(e, sampler._GraphedChain)]


@pytest.mark.parametrize("objective,name", CHAINS, ids=[f"{o}-{k}" for o, k in CHAINS])
def test_chains_match_reference_fixture_and_graph_replay_equals_eager(fx, nets, dev, parity, monkeypatch, objective, name):
    from lgm_hip import sampler
    spec = KINDS[name]
    net = nets[spec.get("net", "plain")]
    gd = _diffusion(fx, net, objective, name, dev)
    net.prepare_hip(dev)
    plan, jump, known, mask, init, trips = _inputs(fx, name, gd, dev)
    guided = spec.get("net") == "guided"
    y = torch.as_tensor(fx["classes"]).to(dev) if guided else None
    scale = float(fx["cond_scale"]) if guided else 1.0
    assert len(plan.times) == {(5, 2): 35, (3, 2): 19, (1, 1): 10}[jump]

    def run():
        return sampler.inpaint(gd, known, mask[:, None], *jump, init_noise=init, noises=trips, classes=y, cond_scale=scale).clone()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = run()
    keys = _inpaint_keys(net)
    want_key = ("inpaint",) + sampler._graph_key(gd, tuple(known.shape), plan.with_noise, plan.rederive, guided, plan.dpm)
    assert want_key in keys, f"graph capture of the inpainting step did not happen: {keys}"
    again = run()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run()
    what = f"{objective}: inpainting chain, {name}"
    assert torch.isfinite(graph).all() and float(graph.std()) > 0
    assert torch.equal(graph, eager), f"{what}: graph replay differs from eager launches"
    assert torch.equal(graph, again), f"{what}: the second chain on one captured step differs from the first"
    _arbiter(parity, f"{what}, final image", graph, fx[f"{objective}:{name}"], unpack64(fx, f"{objective}:{name}"))
    keep = (mask[:, None] == 1).expand_as(graph)
    assert float((graph - torch.as_tensor(fx["known"]).to(dev))[keep].abs().max()) <= 1e-6, "the known region is the given image"
    assert float(graph.min()) >= -1e-6 and float(graph.max()) <= 1 + 1e-6


@pytest.mark.parametrize("name", ["ancestral", "ode2m"])
def test_a_walk_longer_than_the_tables_is_replayed_in_segments(fx, nets, dev, monkeypatch, name):
    """a captured step with tables of 4 rows: 35 / 19 steps go through 9 / 5 segments and come out as the eager chain's bits"""
    from lgm_hip import sampler
    net = nets["plain"]
    gd = _diffusion(fx, net, "pred_v", name, dev)
    net.prepare_hip(dev)
    plan, jump, known, mask, init, trips = _inputs(fx, name, gd, dev)
    shape = tuple(known.shape)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = sampler.inpaint(gd, known, mask[:, None], *jump, init_noise=init, noises=trips)
    gc = sampler._GraphedChain(gd, shape, plan.with_noise, plan.rederive, max_steps=4, dpm=plan.dpm, inpaint=True)
    assert len(sampler._segments(len(plan.times), gc.max_steps)) == -(-len(plan.times) // 4) > 1
    assert tuple(gc.table.shape) == (4, 8) and tuple(gc.itable.shape) == (4, 4)
    chain = sampler._Chain(gd, shape, init, known=known, mask=mask)
    chain.x = gc.run(chain.x, plan.times, plan.rows, trips, inpaint=(chain.known, chain.mask, plan.irows))
    assert torch.equal(chain.image(True), eager), "a segmented replay differs from eager launches"
    assert int(gc.counter.item()) == len(plan.times) - 4 * (len(sampler._segments(len(plan.times), 4)) - 1)


def test_plain_chains_beside_inpainting_chains_keep_their_bits(fx, dev, monkeypatch):
    """a DDIM chain and a dpm++ chain before and after inpainting chains on the same network: the same bits, under their old
    cache keys; the inpainting steps have keys of their own"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    net = Unet(dim=16, channels=3)
    net.load_state_dict(OD.unet_init(dim=16, channels=3, seed=int(fx["seed"])), strict=True)
    mk = lambda **kw: GaussianDiffusion(net, img_size=16, sampling_timesteps=6, **kw).to(dev)  # noqa: E731
    ddim, dpm = mk(), mk(sampler="dpm++")
    net.prepare_hip(dev)
    shape = (2, 3, 16, 16)
    g = torch.Generator().manual_seed(6)
    init = torch.randn(shape, generator=g).to(dev)
    known = torch.rand(shape, generator=g).to(dev)
    mask = torch.zeros(2, 1, 16, 16, device=dev)
    mask[:, :, :, :8] = 1.0
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    both = lambda: (sampler.ddim_sample(ddim, shape, init_noise=init).clone(),  # noqa: E731
                    sampler.dpm_solver_sample(dpm, shape, init_noise=init).clone())
    before = both()
    old_keys = set(sampler._GRAPHS[net])
    assert old_keys == {((2, 3, 16, 16), False), ("dpm++", "pred_v", (2, 3, 16, 16), False)}, "the existing keys are unchanged"
    torch.manual_seed(1)
    filled = (ddim.inpaint(known, mask, jump_length=2, resamples=2).clone(), dpm.inpaint(known, mask, jump_length=2, resamples=2).clone())
    assert set(_inpaint_keys(net)) == {("inpaint",) + k for k in old_keys} and len(sampler._GRAPHS[net]) == 4
    after = both()
    for a, b, c in zip(before, after, filled):
        assert torch.equal(a, b), "a plain chain changed its bits beside an inpainting one"
        assert torch.isfinite(c).all() and not torch.equal(a, c)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = both()
    assert torch.equal(eager[0], before[0]) and torch.equal(eager[1], before[1])


def test_public_inpaint(nets, dev, monkeypatch):
    """``GaussianDiffusion.inpaint`` on the three samplers, soft and binary masks in both layouts, a guided and thresholded and
    a self-conditioned network beside the plain one; ``DDPM.inpaint`` reaches the EMA diffusion's"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import DDPM, GaussianDiffusion
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    g = torch.Generator().manual_seed(12)
    known = torch.rand(2, 3, 16, 16, generator=g).to(dev)
    mask = torch.zeros(2, 16, 16, device=dev)
    mask[0, 4:12, 4:12], mask[1, :, ::2] = 1.0, 1.0
    keep = (mask[:, None] == 1).expand_as(known)
    shape = (2, 3, 16, 16)
    outs = {}
    for name, kw, key in (("ancestral", dict(timesteps=8), ("inpaint", shape, True)),
                          ("ddim", dict(timesteps=1000, sampling_timesteps=4), ("inpaint", shape, False)),
                          ("dpm++", dict(timesteps=1000, sampling_timesteps=4, sampler="dpm++"),
                           ("inpaint", "dpm++", "pred_v", shape, False))):
        for kind in {"ancestral": ("plain", "guided"), "ddim": ("plain", "selfcond"), "dpm++": ("plain",)}[name]:
            net = nets[kind]
            net.prepare_hip(dev)
            gd = GaussianDiffusion(net, img_size=16, dynamic_thresholding=kind == "guided", **kw).to(dev)
            extra = dict(classes=torch.tensor([1, 4], device=dev), cond_scale=2.0) if kind == "guided" else {}
            for m in ((mask, mask[:, None]) if kind == "plain" else (mask,)):
                torch.manual_seed(4)
                out = gd.inpaint(known, m, jump_length=2, resamples=2, **extra)
                assert out.shape == known.shape and torch.isfinite(out).all()
                assert float(out.min()) >= -1e-6 and float(out.max()) <= 1 + 1e-6, "inside the data range"
                assert float((out - known)[keep].abs().max()) <= 1e-6, (name, kind)
                assert not torch.equal(out[~keep], known[~keep])
            if kind == "plain":
                assert key in _inpaint_keys(net), (name, _inpaint_keys(net))       # dispatch follows sampler=
                torch.manual_seed(4)
                frames = gd.inpaint(known, mask, jump_length=2, resamples=2, return_all_timesteps=True)
                n = len(sampler._plan_inpaint(gd, 2, 2).times)
                assert tuple(frames.shape) == (2, n + 1, 3, 16, 16) and torch.isfinite(frames).all()
                outs[name] = out
                soft = torch.full((2, 1, 16, 16), 0.5, device=dev)
                mid = gd.inpaint(known, soft)
                assert torch.isfinite(mid).all() and float(mid.min()) >= -1e-6 and float(mid.max()) <= 1 + 1e-6
    assert not torch.equal(outs["ddim"], outs["dpm++"]) and not torch.equal(outs["ddim"], outs["ancestral"])
    with pytest.raises(ValueError):
        gd.inpaint(known, mask * 2)
    torch.manual_seed(0)
    m = DDPM(img_channels=3, img_size=16, dim=16, diffusion_timesteps=8).to(dev)
    m.prepare_hip(dev)
    torch.manual_seed(5)
    a = m.inpaint(known, mask, jump_length=2, resamples=2)
    torch.manual_seed(5)
    b = m.ema.ema_model.inpaint(known, mask, jump_length=2, resamples=2)
    assert torch.equal(a, b) and float((a - known)[keep].abs().max()) <= 1e-6
