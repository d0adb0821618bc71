"""GPU: the variational-bound likelihood in bits per dimension on the HIP path (``GaussianDiffusion.vlb_terms`` / ``nll_bpd``;
Ho et al. 2020 eq. 5, Nichol & Dhariwal 2021 ``calc_bpd_loop``, an extension of the reference): ``vlb_term_kernel`` behind
``lgm_vlb_term`` / ``lgm_vlb_term_table`` and the graph-replayed evaluation of lgm_hip/likelihood.py.

  * KL rows at t in {999, 500, 1}, the decoder row on crafted inputs and the prior row against float64 from the same float32
    operands and row, 1e-4 relative per sample (the project's RTOL), at the smallest shapes that can go wrong; lanes and output
    rows the kernel must not touch hold NaN;
  * the table form against the by-value form bit for bit;
  * evaluations against tests/golden/diffusion_bpd.npz (tools/make_golden_bpd.py: the textbook formulas around the REFERENCE's
    network), every evaluated timestep's row on its own at 1e-4 relative with the float64 arbiter rule of
    tests/test_hip_dynthresh.py;
  * graph replay bit for bit against eager launches under injected draws, a second replay, more timesteps than table rows;
    sampling chains before and after an evaluation keep their bits and keys; drawn noise; the public methods.

Why 1e-4 holds for a KL row.  Per element the kernel rounds x0_pred (<= 3 roundings relative to the magnitudes of its two
products), d0 = x0_pred - x0, d = P1 d0 and d^2: with x0_pred and x0 drawn independently |d0| is O(1) against operands that
are O(1) (clipped) or up to O(R |x|), in the thousands (pred_noise at t = 999, unclipped, where d0 is of that size too), so
every element's d^2 carries a few 2^-24 relative and the 75 ... 900 terms of a sample's sum at most n 2^-24 more: below 1e-5
in all.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4
NAN = float("nan")
LN2 = math.log(2.0)
# (B, C, HW, pitch, x_off, sc_off): the three of tests/test_hip_inpaint.py, and one in which a workgroup's pixel loop (256
# lanes) runs two trips, the second with 44 pixels
GEOMS = [(3, 3, 25, 4, 0, -1), (3, 3, 25, 8, 3, 0), (3, 1, 25, 4, 0, -1), (2, 3, 300, 4, 0, -1)]
GIDS = ["3x3x25", "selfcond_3x3x25", "3x1x25", "2x3x300"]
N_ROWS, AT = 3, 1                                   # the output has three rows, the launches address the middle one


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_bpd.npz")))


@pytest.fixture(scope="module")
def plans():
    """{variance: {t: row}} of a T = 1000 diffusion (sigmoid schedule), and the prior row"""
    from lgm_hip import likelihood as LK
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)
    ts = [999, 500, 1, 0]
    out = {}
    for variance in LK.VARIANCES:
        rows = LK.vlb_plan(gd, ts, variance)
        out[variance] = dict(zip(ts, rows[:4]))
        out["prior"] = rows[4]
    return out


def _r4(n):
    return (n + 3) // 4 * 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _operands(seed, geom):
    """host operands with NaN wherever the kernel must not read: pad lanes and the self-conditioning slice of the input
    buffer, pad lanes of the network output.  img in [0, 1] on the 8-bit grid (normalised by the kernel)"""
    B, C, HW, pitch, x_off, sc_off = geom
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, C, HW), generator=g).float() / 255.0
    noise = torch.randn(B, C, HW, generator=g)
    xin = torch.full((B, HW, pitch), NAN)
    xin[..., x_off:x_off + C] = torch.randn(B, HW, C, generator=g) * 1.5
    v = torch.full((B, HW, _r4(C)), NAN)
    v[..., :C] = torch.randn(B, HW, C, generator=g)
    return dict(img=img, noise=noise, xin=xin, v=v)


def _launch(geom, d, objective, clip, row, normalize=1, out=None, at=AT, table=None, counter=None, stride=12, advance=0,
            prior=False):
    """one launch on the device operands ``d`` -> the [N_ROWS, 3, B] output, NaN wherever the launch did not write"""
    from lgm_hip import likelihood as LK, ops
    B, C, HW, pitch, x_off, sc_off = geom
    L = ops.lib()
    if out is None:
        out = torch.full((N_ROWS, 3, B), NAN, device=d["img"].device)
    src = (d["img"].data_ptr(), None if prior else d["noise"].data_ptr(), normalize, None if prior else d["xin"].data_ptr(),
           pitch, x_off, None if prior else d["v"].data_ptr(), _r4(C), B, C, HW, objective, 1 if clip else 0)
    if table is not None:
        L.lgm_vlb_term_table(*src, table.data_ptr(), stride, counter.data_ptr(), out.data_ptr(), N_ROWS, advance, ops.stream())
    else:
        L.lgm_vlb_term(*src, *LK._byval(row), out.data_ptr(), N_ROWS, at, ops.stream())
    assert L._dll.lgm_last_kernel().decode() == "vlb_term_kernel"
    return out


def _predictions64(geom, h, objective, clip, row, normalize=True):
    """model_predictions' branch in float64 from the float32 operands -> (x0, x_t, x0_pred, eps_pred, noise), [B, HW, C]"""
    B, C, HW, pitch, x_off, sc_off = geom
    A, S, R, Rm1 = row[:4]
    x0 = h["img"].double().permute(0, 2, 1)
    x0 = x0 * 2 - 1 if normalize else x0
    x, ov = h["xin"][..., x_off:x_off + C].double(), h["v"][..., :C].double()
    x0p = {0: R * x - Rm1 * ov, 1: ov, 2: A * x - S * ov}[objective]
    if clip:
        x0p = x0p.clamp(-1.0, 1.0)
    eps = ov if (objective == 0 and not clip) else (R * x - x0p) / Rm1
    return x0, x, x0p, eps, h["noise"].double().permute(0, 2, 1)


def _only_row(out, at):
    """the addressed row; every other row of the output still holds NaN"""
    o = out.cpu()
    other = [i for i in range(o.shape[0]) if i != at]
    assert torch.isnan(o[other]).all(), "a row that was not addressed has been written"
    assert torch.isfinite(o[at]).all()
    return o[at].double()


def _worst(got, want):
    return float(((got - want).abs() / want.abs()).max())


@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_kl_rows_against_float64(dev, plans, parity, geom):
    worst = {"vb": 0.0, "xstart_mse": 0.0, "mse": 0.0}
    for variance in ("fixed_small", "fixed_large"):
        for t in (999, 500, 1):
            row = plans[variance][t]
            assert int(row[6]) == 0 and (row[7] == 0.0) == (variance == "fixed_small")
            for objective in (0, 1, 2):
                for clip in (False, True):
                    h = _operands(10000 * objective + 10 * t + clip, geom)
                    d = {k: a.to(dev) for k, a in h.items()}
                    got = _only_row(_launch(geom, d, objective, clip, row), AT)
                    x0, x, x0p, eps, nz = _predictions64(geom, h, objective, clip, row)
                    dd = row[4] * (x0p - x0)
                    want = torch.stack([(row[7] + row[8] * (dd ** 2).flatten(1).mean(1)) / LN2,
                                        ((x0p - x0) ** 2).flatten(1).mean(1), ((eps - nz) ** 2).flatten(1).mean(1)])
                    what = (variance, t, objective, clip)
                    assert float((x0p - x0).abs().mean()) > 0.3, (what, "the difference is O(1)")
                    for k, name in enumerate(worst):
                        e = _worst(got[k], want[k])
                        worst[name] = max(worst[name], e)
                        assert e < RTOL, (what, name, e, got[k].tolist(), want[k].tolist())
    for name, e in worst.items():
        parity(f"vlb_term KL rows {GIDS[GEOMS.index(geom)]}: {name}, worst sample against float64", e, RTOL)


LOG_SIGMAS = (-4.4, -3.0, -1.0, 0.0)
FIXED_Z = (0.0, 4.6, 5.5, 6.1, -6.1, 7.5)


def _decoder64(x, mean, inv_std):
    """Nichol & Dhariwal's discretized_gaussian_log_likelihood, the textbook form, in float64"""
    cdf = lambda z: 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))  # noqa: E731
    c = x - mean
    plus, minus = cdf(inv_std * (c + 1.0 / 255.0)), cdf(inv_std * (c - 1.0 / 255.0))
    lp, lm = torch.log(plus.clamp(min=1e-12)), torch.log((1.0 - minus).clamp(min=1e-12))
    ld = torch.log((plus - minus).clamp(min=1e-12))
    return torch.where(x < -0.999, lp, torch.where(x > 0.999, lm, ld))


@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_decoder_row_against_float64_on_crafted_inputs(dev, plans, parity, geom):
    """images on the 8-bit grid with exactly +-1 and +-(1 - 2/255) among them, standardised residuals uniform in [-9, 9] plus
    FIXED_Z, four sigmas; pred_x0 without clipping, so that the network output IS x0_pred and the mean P1 x0_pred + P2 x_t
    lands where the residual wants it.  With 75 elements per sample one wrongly floored element moves the sum by about 1 %."""
    B, C, HW, pitch, x_off, sc_off = geom
    P1, P2 = 0.75, 0.25
    base = plans["fixed_small"][0]
    assert int(base[6]) == 1
    worst, floored, tail = 0.0, 0, 0
    for ls in LOG_SIGMAS:
        sigma = math.exp(ls)
        inv_std = float(np.float32(1.0 / sigma))
        g = torch.Generator().manual_seed(int(-10 * ls) + 7)
        h = _operands(int(-10 * ls), geom)
        x = torch.randint(0, 256, (B, HW, C), generator=g).double() / 255.0 * 2 - 1
        x[:, :4, 0] = torch.tensor([-1.0, 1.0, -(1.0 - 2.0 / 255.0), 1.0 - 2.0 / 255.0], dtype=torch.float64)
        z = torch.rand(B, HW, C, generator=g).double() * 18 - 9
        z[:, 4:4 + len(FIXED_Z), 0] = torch.tensor(FIXED_Z, dtype=torch.float64)
        xt = h["xin"][..., x_off:x_off + C].double().clamp(-1, 1)
        h["xin"][..., x_off:x_off + C] = xt.float()
        h["v"][..., :C] = (((x - z * sigma) - P2 * xt) / P1).float()
        h["img"] = x.float().permute(0, 2, 1).contiguous()
        row = base[:4] + (P1, P2, 1.0, 0.0, 0.0, inv_std, 0.0, 0.0)
        d = {k: a.to(dev) for k, a in h.items()}
        got = _only_row(_launch(geom, d, 1, False, row, normalize=0), AT)
        x0, xv, x0p, eps, nz = _predictions64(geom, h, 1, False, row, normalize=False)
        logp = _decoder64(x0, P1 * x0p + P2 * xv, inv_std)
        zz = inv_std * (x0 - (P1 * x0p + P2 * xv))
        floored += int((logp <= math.log(1e-12) + 1e-9).sum())
        tail += int(((zz.abs() > 4.6) & (logp > math.log(1e-12) + 1e-9)).sum())
        want = torch.stack([-logp.flatten(1).mean(1) / LN2, ((x0p - x0) ** 2).flatten(1).mean(1),
                            ((eps - nz) ** 2).flatten(1).mean(1)])
        e = _worst(got[0], want[0])
        worst = max(worst, e)
        assert e < RTOL, (ls, e, got[0].tolist(), want[0].tolist())
        assert _worst(got[1], want[1]) < RTOL and _worst(got[2], want[2]) < RTOL
    assert floored > 0 and tail > 0, "the inputs reach the floor and the zone in which float32's 1 - tanh has no bits left"
    parity(f"vlb_term decoder row {GIDS[GEOMS.index(geom)]}: worst sample against float64", worst, RTOL)


@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_prior_row_against_float64(dev, plans, parity, geom):
    row = plans["prior"]
    assert int(row[6]) == 2
    h = _operands(5, geom)
    d = {k: a.to(dev) for k, a in h.items()}
    for normalize in (1, 0):
        out = _launch(geom, d, 2, True, row, normalize=normalize, prior=True)
        got = _only_row(out, AT)
        x0 = h["img"].double() * 2 - 1 if normalize else h["img"].double()
        want = (row[7] + row[8] * (x0 ** 2).flatten(1).mean(1)) / LN2
        a = row[10]
        closed = (0.5 * (-1.0 - math.log1p(-a) + (1.0 - a) + a * x0 ** 2)).flatten(1).mean(1) / LN2
        assert _worst(want, closed) < 1e-6, "the row's (KC, KW) are the closed form's"
        parity(f"vlb_term prior row {GIDS[GEOMS.index(geom)]} normalize={normalize}", _worst(got[0], want), RTOL)
        assert _worst(got[0], closed) < RTOL
        assert torch.equal(out[AT, 1:].cpu(), torch.zeros(2, geom[0])), "outputs [1] and [2] of a prior row are exactly 0"


@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_table_form_equals_by_value_form(dev, plans, geom):
    """row counter[0] of the table into output row counter[0]; advance moves the counter; a wider stride; a counter outside
    the output writes nothing"""
    B = geom[0]
    for objective in (0, 2):
        for t, variance, stride in ((999, "fixed_large", 12), (1, "fixed_small", 16), (0, "fixed_small", 12)):
            row = plans[variance][t]
            h = _operands(31 * objective + t, geom)
            d = {k: a.to(dev) for k, a in h.items()}
            for at in (0, 2):
                want = _launch(geom, d, objective, True, row, at=at)
                table = torch.full((N_ROWS, stride), 0.25)
                table[at, :12] = torch.tensor(row)
                counter = torch.full((1,), at, dtype=torch.int32, device=dev)
                got = _launch(geom, d, objective, True, None, table=table.to(dev), counter=counter, stride=stride, advance=1)
                _only_row(got, at)
                assert torch.equal(_bits(got[at]), _bits(want[at])), (objective, t, at)
                assert int(counter.item()) == at + 1
                same = _launch(geom, d, objective, True, None, table=table.to(dev), counter=counter, stride=stride, advance=0)
                assert int(counter.item()) == at + 1, "no advance: the counter stays"
                if at + 1 < N_ROWS:
                    assert torch.isfinite(same[at + 1]).all()
                else:
                    assert torch.isnan(same).all(), "a counter past the output writes nothing"
    assert B > 0


# ----------------------------------------------------------------------------------------------------------------------
# evaluations against the reference fixture; graph replay against eager launches
# ----------------------------------------------------------------------------------------------------------------------
CASES = {"pred_v:small": ("pred_v", "fixed_small", True, "plain"), "pred_v:large": ("pred_v", "fixed_large", True, "plain"),
         "pred_noise:small": ("pred_noise", "fixed_small", True, "plain"),
         "pred_noise:large": ("pred_noise", "fixed_large", True, "plain"), "pred_v:noclip": ("pred_v", "fixed_small", False, "plain"),
         "pred_v:selfcond": ("pred_v", "fixed_small", True, "selfcond"), "pred_v:labels": ("pred_v", "fixed_small", True, "labels")}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def nets(fx, dev):
    """the three networks of the fixture, built once"""
    from models.generative.diffusion.ddpm import Unet
    from oracle import diffusion as OD
    P = OD.unet_init(dim=int(fx["dim"]), channels=3, seed=int(fx["seed"]))
    out = {}
    for kind, kw, extra in (("plain", {}, {}),
                            ("selfcond", dict(self_condition=True), {"init_conv.weight": fx["sc:init_conv.weight"]}),
                            ("labels", dict(num_classes=int(fx["K"])), {"label_emb.weight": fx["label_emb.weight"]})):
        net = Unet(dim=int(fx["dim"]), channels=3, **kw)
        net.load_state_dict(dict(P, **{k: torch.as_tensor(v) for k, v in extra.items()}), strict=True)
        out[kind] = net
    return out


def _arbiter_rows(parity, what, hip, ref, exact):
    """every row (evaluated timestep) on its own: 1e-4 against the reference's float32 result; a miss is decided by float64 -
    HIP no further from it than twice the reference itself.  The worst row's three distances go on record."""
    hip, ref, exact = (torch.as_tensor(a).double().cpu().reshape(-1, hip.shape[-1]) for a in (hip, ref, exact))
    worst = (-1.0, 0.0, 0.0, 0)
    for i in range(hip.shape[0]):
        e, d_ref, d_hip = rel(hip[i], ref[i]), rel(ref[i], exact[i]), rel(hip[i], exact[i])
        worst = max(worst, (e, d_ref, d_hip, i))
        if e >= RTOL:
            print(f"[parity] {what} row {i}: |hip-ref| {e:.3e} misses {RTOL:.0e}; distance to float64: reference {d_ref:.3e}, "
                  f"hip {d_hip:.3e}")
            assert d_hip <= 2 * d_ref, (what, i, e, d_hip, d_ref)
    parity.record(what + " [worst row, distances to float64]", hip_vs_ref=worst[0], ref_vs_fp64=worst[1], hip_vs_fp64=worst[2],
                  row=worst[3])


def _evaluate(fx, nets, dev, case, steps, **kw):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    from oracle import diffusion as OD
    objective, variance, clip, kind = CASES[case]
    net = nets[kind]
    gd = GaussianDiffusion(net, img_size=int(fx["S"]), timesteps=steps, objective=objective).to(dev)
    net.prepare_hip(dev)
    times = [int(t) for t in fx["times"]] if steps == int(fx["T"]) else None
    n = len(times) if times is not None else steps
    shape = (int(fx["B"]), 3, int(fx["S"]), int(fx["S"]))
    _, nz = OD.draw_loop_noise(int(fx[f"{case}_seed"]), shape, n)
    y = torch.as_tensor(fx["classes"]).to(dev) if kind == "labels" else None
    img = torch.as_tensor(fx["img"]).to(dev)
    run = lambda: gd.vlb_terms(img, timesteps=times, noise=[z.to(dev) for z in nz], clip_denoised=clip,  # noqa: E731
                               variance=variance, classes=y, **kw)
    return gd, run


@pytest.mark.parametrize("steps", [1000, 20])
@pytest.mark.parametrize("case", list(CASES))
def test_evaluations_match_reference_fixture_and_graph_replay_equals_eager(fx, nets, dev, parity, monkeypatch, case, steps):
    from lgm_hip import likelihood as LK, sampler
    gd, run = _evaluate(fx, nets, dev, case, steps)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = run()
    key = LK._vlb_key(gd, (int(fx["B"]), 3, int(fx["S"]), int(fx["S"])), CASES[case][2])
    assert isinstance(sampler._GRAPHS[gd.model].get(key), LK._GraphedVLB), "graph capture of the evaluation step did not happen"
    again = run()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run()
    n = 8 if steps == 1000 else 20
    assert graph.timesteps == (tuple(int(t) for t in fx["times"]) if steps == 1000 else tuple(reversed(range(20))))
    for name in ("vb", "xstart_mse", "mse", "prior_bpd"):
        a, b, c = getattr(graph, name), getattr(eager, name), getattr(again, name)
        assert a.dtype == torch.float64 and tuple(a.shape) == ((n, 4) if name != "prior_bpd" else (4,))
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"{case}: {name}: graph replay differs from eager launches"
        assert torch.equal(a, c), f"{case}: {name}: the second evaluation on one captured step differs from the first"
        k = f"{case}:{steps}:{'prior' if name == 'prior_bpd' else name}"
        _arbiter_rows(parity, f"{case}, T = {steps}: {name}", a, fx[k], fx[k + "64"])
    if steps == 20:
        assert graph.total_bpd is not None and tuple(graph.total_bpd.shape) == (4,)
        want = graph.vb.sum(0) + graph.prior_bpd
        assert float(((graph.total_bpd - want).abs() / want).max()) <= 1e-14, "total_bpd = vb.sum(0) + prior_bpd"
        _arbiter_rows(parity, f"{case}, T = 20: total_bpd", graph.total_bpd, fx[f"{case}:20:total"], fx[f"{case}:20:total64"])
    else:
        assert graph.total_bpd is None, "a subset has no total"


def test_more_timesteps_than_table_rows_are_replayed_in_segments(fx, nets, dev, monkeypatch):
    """a captured step with tables of 3 rows: 8 timesteps go through 3 segments and come out as the eager loop's bits"""
    from lgm_hip import likelihood as LK, sampler
    from oracle import diffusion as OD
    gd, run = _evaluate(fx, nets, dev, "pred_v:large", 1000)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run()
    times = [int(t) for t in fx["times"]]
    shape = (int(fx["B"]), 3, int(fx["S"]), int(fx["S"]))
    gv = LK._GraphedVLB(gd, shape, True, max_steps=3)
    assert tuple(gv.table.shape) == (3, LK.VLB_ROW) and tuple(gv.out.shape) == (3, 3, 4)
    assert len(sampler._segments(len(times), gv.max_steps)) == 3
    _, nz = OD.draw_loop_noise(int(fx["pred_v:large_seed"]), shape, len(times))
    rows = LK.vlb_plan(gd, times, "fixed_large")
    img = torch.as_tensor(fx["img"]).to(dev)
    got = gv.run(gd, img, times, rows[:-1], [z.to(dev) for z in nz]).double().cpu()
    assert torch.equal(got[:, 0], eager.vb) and torch.equal(got[:, 1], eager.xstart_mse) and torch.equal(got[:, 2], eager.mse)
    assert int(gv.counter.item()) == 2


def test_sampling_chains_beside_an_evaluation_keep_their_bits(fx, dev, monkeypatch):
    """a DDIM chain and a dpm++ chain before and after an evaluation on the same network: the same bits, under their old
    cache keys; the evaluation step has a key of its own"""
    from lgm_hip import likelihood as LK, sampler
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
    img = torch.rand(shape, generator=g).to(dev)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    both = lambda: (sampler.ddim_sample(ddim, shape, init_noise=init).clone(),  # noqa: E731
                    sampler.dpm_solver_sample(dpm, shape, init_noise=init).clone())
    before = both()
    old_keys = set(sampler._GRAPHS[net])
    assert old_keys == {((2, 3, 16, 16), False), ("dpm++", "pred_v", (2, 3, 16, 16), False)}, "the existing keys are unchanged"
    torch.manual_seed(1)
    res = ddim.vlb_terms(img, timesteps=[999, 400, 0])
    assert torch.isfinite(res.vb).all() and res.total_bpd is None
    assert set(sampler._GRAPHS[net]) == old_keys | {LK._vlb_key(ddim, shape, True)}
    after = both()
    for a, b in zip(before, after):
        assert torch.equal(a, b), "a sampling chain changed its bits beside an evaluation"


def test_evaluation_step_is_recaptured_when_the_parameter_storage_is_replaced(fx, dev, monkeypatch):
    """the likelihood's twin of tests/test_hip_unet.py's invalidation: after every parameter got new storage prepare_hip()
    rebuilds the flat buffers, the step captured against the old ones is dropped and recaptured, and the evaluation reads the
    NEW weights (a stale graph would go on reading the old buffers)"""
    from lgm_hip import likelihood as LK, sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    net = Unet(dim=16, channels=3)
    net.load_state_dict(OD.unet_init(dim=16, channels=3, seed=int(fx["seed"])), strict=True)
    gd = GaussianDiffusion(net, img_size=16, timesteps=12).to(dev)
    shape = (2, 3, 16, 16)
    g = torch.Generator().manual_seed(9)
    img = torch.rand(shape, generator=g).to(dev)
    nz = [torch.randn(shape, generator=g).to(dev) for _ in range(2)]
    run = lambda: gd.vlb_terms(img, timesteps=[5, 0], noise=nz)  # noqa: E731
    key = LK._vlb_key(gd, shape, True)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    first = run()
    old = sampler._GRAPHS[net].get(key)
    assert isinstance(old, LK._GraphedVLB), "graph capture of the evaluation step did not happen"
    with torch.no_grad():
        for p in net.parameters():
            p.data = (p.data * 1.01).clone()            # new storage, different values
    assert not net._flat.still_bound()
    second = run()
    new = sampler._GRAPHS[net][key]
    assert isinstance(new, LK._GraphedVLB) and new is not old and new.matches(net)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run()
    for name in ("vb", "xstart_mse", "mse", "prior_bpd"):
        assert torch.equal(getattr(second, name), getattr(eager, name)), f"{name}: the recaptured step differs from eager launches"
    assert not torch.equal(second.vb, first.vb), "the evaluation still reads the old weights"


def test_drawn_noise_and_the_public_methods(nets, dev, monkeypatch):
    """``noise=None``: two calls under one seed agree and capture leaves the random stream where it was; ``nll_bpd``,
    ``DDPM.bits_per_dim`` and ``validation_step`` under ``bpd_every``; shape mismatches raise"""
    from lgm_hip import likelihood as LK
    from models.generative.diffusion.ddpm import DDPM, GaussianDiffusion
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    net = nets["plain"]
    net.prepare_hip(dev)
    gd = GaussianDiffusion(net, img_size=16, timesteps=12, objective="pred_noise").to(dev)
    img = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    torch.manual_seed(11)
    state = torch.cuda.get_rng_state(dev)
    gv = LK._GraphedVLB(gd, (2, 3, 16, 16), True)
    assert torch.equal(torch.cuda.get_rng_state(dev), state), "capture moved the random stream"
    del gv
    torch.manual_seed(11)
    a = gd.vlb_terms(img)
    torch.manual_seed(11)
    b = gd.vlb_terms(img)
    torch.manual_seed(12)
    c = gd.vlb_terms(img)
    assert torch.equal(a.vb, b.vb) and torch.equal(a.total_bpd, b.total_bpd) and not torch.equal(a.vb, c.vb)
    assert tuple(a.vb.shape) == (12, 2) and a.timesteps == tuple(reversed(range(12))) and bool((a.total_bpd > 0).all())
    assert torch.equal(a.prior_bpd, c.prior_bpd), "the prior reads the image only"
    torch.manual_seed(11)
    assert torch.equal(gd.nll_bpd(img), a.total_bpd)
    small, large = gd.vlb_terms(img, variance="fixed_small", timesteps=[5]), gd.vlb_terms(img, variance="fixed_large", timesteps=[5])
    assert torch.isfinite(small.vb).all() and torch.isfinite(large.vb).all()
    for bad in (dict(noise=[img]), dict(noise=[img[:1]] * 12), dict(variance="learned"), dict(timesteps=[12])):
        with pytest.raises(ValueError):
            gd.vlb_terms(img, **bad)
    with pytest.raises(ValueError):
        gd.vlb_terms(img[:, :, :8])
    with pytest.raises(ValueError):
        gd.vlb_terms(img, classes=torch.zeros(2, dtype=torch.long))
    # the self-conditioned and the class-conditional network through the public method
    for kind, kw in (("selfcond", {}), ("labels", dict(classes=torch.tensor([1, 4])))):
        g2 = GaussianDiffusion(nets[kind], img_size=16, timesteps=6).to(dev)
        r = g2.vlb_terms(img, **kw)
        assert torch.isfinite(r.total_bpd).all()
        if kw:
            torch.manual_seed(2)
            null = g2.nll_bpd(img)
            torch.manual_seed(2)
            cond = g2.nll_bpd(img, **kw)
            assert not torch.equal(null, cond), "labels give the conditional bound"
    torch.manual_seed(0)
    m = DDPM(img_channels=3, img_size=16, dim=16, diffusion_timesteps=8).to(dev)
    m.prepare_hip(dev)
    m.sample_every = 0
    torch.manual_seed(5)
    x = m.bits_per_dim(img)
    torch.manual_seed(5)
    y = m.ema.ema_model.nll_bpd(img)
    assert torch.equal(x, y) and tuple(x.shape) == (2,) and not m.ema.ema_model.training
    logs = []
    m.log = lambda name, value, **kw: logs.append((name, float(value)))
    m.eval()
    m.bpd_every = 1
    m.validation_step((img, torch.zeros(2, dtype=torch.long)))
    assert [n for n, _ in logs] == ["val_loss", "val_bpd"] and all(math.isfinite(v) for _, v in logs)
