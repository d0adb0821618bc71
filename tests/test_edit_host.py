"""CPU: the host side of DDIM inversion, img2img and the slerp interpolation (lgm_hip.sampler, GaussianDiffusion.encode /
decode / reconstruct / img2img / interpolate(method="ddim")).  Plans and rows against the float64 restatements of
tests/edit_ref.py, the algebraic round trip the inverse plan rests on, the truncated img2img plans, every refusal, the graph
cache keys (the existing ones unchanged), the new C symbols and the fixture tools/make_golden_edit.py wrote.  No device."""
import os

import numpy as np
import pytest
import torch

import edit_ref

U = 2.0 ** -24


def _gd(T=1000, steps=None, net_kw=None, **kw):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    return GaussianDiffusion(Unet(dim=16, channels=3, **(net_kw or {})), img_size=8, timesteps=T, sampling_timesteps=steps, **kw)


GRIDS = [(8, 3), (8, 7), (8, 8), (50, 5), (50, 49), (1000, 10), (1000, 11), (1000, 21), (1000, 250)]


@pytest.mark.parametrize("T,N", GRIDS, ids=[f"T{t}-N{n}" for t, n in GRIDS])
def test_inverse_pairs_and_rows(T, N):
    """The pairs: ascending, contiguous, from the grid's lowest level to T - 1, ``upto`` a prefix.  The rows: the head and
    sqrt(acp_u) are the float64 value rounded ONCE (a float32 root of a float32 number is that); sqrt(1 - acp_u) is formed as
    the reference forms it, 1 - acp_u and its root both in float32: two roundings, each at most u relative, the first halved
    by the root - asserted within 2 u of the float64 value."""
    from lgm_hip import sampler
    gd = _gd(T, N if N < T else None)
    kw = dict(steps=N) if N == T else {}
    pairs = sampler.ddim_inverse_pairs(gd, **kw)
    grid = edit_ref.inverse_grid(T, N)
    assert grid == sorted({t for t, _ in gd.ddim_time_pairs(N)}) and len(grid) == N
    assert pairs == list(zip(grid[:-1], grid[1:])) and len(pairs) == N - 1
    assert all(u > t for t, u in pairs) and all(a[1] == b[0] for a, b in zip(pairs, pairs[1:]))
    assert pairs[-1][1] == T - 1 and pairs[0][0] == grid[0]
    for k in {1, max(1, (N - 1) // 2), N - 1}:
        assert sampler.ddim_inverse_pairs(gd, upto=k, **kw) == pairs[:k]
    for bad in (0, N, -1, 1.5):
        with pytest.raises(ValueError, match="upto"):
            sampler.ddim_inverse_pairs(gd, upto=bad, **kw)
    plan = sampler._plan_ddim_inverse(gd, **kw)
    assert plan.times == tuple(t for t, _ in pairs) and not plan.with_noise and not any(plan.draws)
    assert plan.clip is False and plan.rederive and not plan.dpm and plan.irows is None and not plan.learned
    acp32 = gd.alphas_cumprod.double().numpy()                    # the float32 table the library reads, exactly
    exact = {k: getattr(gd, k).double().numpy() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                                          "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")}
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    for (t, u), row in zip(pairs, plan.rows):
        assert len(row) == 8 and row == sampler._ddim_coeffs(gd, t, u, 0.0)
        want = edit_ref.inverse_row(acp32, t, u)
        assert row[0] == f32(exact["sqrt_alphas_cumprod"][t]) and row[1] == -f32(exact["sqrt_one_minus_alphas_cumprod"][t])
        assert row[2] == f32(exact["sqrt_recip_alphas_cumprod"][t]) and row[3] == f32(exact["sqrt_recipm1_alphas_cumprod"][t])
        # (the head: the diffusion's tables, float64 values of the float64 schedule rounded once - not functions of acp32)
        assert row[4] == f32(want[4]) and row[5] == 0.0 and row[7] == 0.0
        assert abs(row[6] - want[6]) <= 2 * U * want[6]
        assert all(np.isfinite(row))


def test_existing_ddim_rows_keep_their_bits():
    """eta == 0 no longer multiplies a root by zero: the rows of the sampling direction are what they were"""
    from lgm_hip import sampler
    gd = _gd(1000, 10)
    hs = sampler._host_schedule(gd)
    for t, s in gd.ddim_time_pairs()[:-1]:
        a, an = hs["alphas_cumprod"][t], hs["alphas_cumprod"][s]
        sigma = 0.0 * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
        old = sampler._head(hs, t) + (sampler._f32(an.sqrt()), 0.0, sampler._f32((1 - an - sigma ** 2).sqrt()), sampler._f32(sigma))
        assert sampler._ddim_coeffs(gd, t, s, 0.0) == old


@pytest.mark.parametrize("T,N", [(8, 5), (50, 10), (1000, 11), (1000, 50)])
def test_round_trip_identity_in_float64(T, N):
    """With an eps that depends neither on x nor on the level the inverse chain followed by the forward chain on the same
    grid is the identity: every move keeps (x0, eps) and re-mixes them (a network is that to first order in the step).  The
    identity the plan rests on, to 1e-10 in float64."""
    gd = _gd(T, N if N < T else None)
    acp = gd.alphas_cumprod.double().numpy()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 4, 4))
    field = rng.standard_normal(x.shape[1:])                      # one eps for every state and level
    eps_fn = lambda x, t: np.broadcast_to(field, x.shape)  # noqa: E731
    g = edit_ref.inverse_grid(T, N)
    up = list(zip(g[:-1], g[1:]))
    z = edit_ref.ddim_inverse_loop(acp, x, up, eps_fn)
    assert np.abs(z - x).max() > 1e-2
    down = [(u, t) for t, u in reversed(up)]
    back = edit_ref.ddim_forward_loop(acp, z, down, eps_fn)
    assert np.abs(back - x).max() <= 1e-10 * max(1.0, np.abs(x).max())
    # ... and the library's own plans are those two chains
    from lgm_hip import sampler
    kw = dict(steps=N) if N == T else {}
    assert sampler._plan_ddim_inverse(gd, **kw).times == tuple(t for t, _ in up)
    dec = sampler._plan_decode(gd, clip=False, **kw)
    assert dec.times == tuple(t for t, _ in down) + (g[0],) and dec.clip is False and not dec.with_noise
    assert sampler._plan_decode(gd, **kw).clip is True
    for L in (0, len(g) // 2, len(g) - 1):
        part = sampler._plan_decode(gd, from_level=L, **kw)
        assert part.times == tuple(g[L::-1]) and part.rows[-1][4:] == (1.0, 0.0, 0.0, 0.0)
    for bad in (-1, len(g), 0.5):
        with pytest.raises(ValueError, match="from_level"):
            sampler._plan_decode(gd, from_level=bad, **kw)


def test_img2img_step_counts_and_truncated_plans():
    from lgm_hip import sampler
    assert [sampler.img2img_steps(10, s) for s in (1e-6, 0.04, 0.5, 0.55, 1.0)] == [1, 1, 5, 6, 10]
    assert sampler.img2img_steps(50, 0.5) == 25 and sampler.img2img_steps(1000, 1.0) == 1000
    for bad in (0.0, -0.1, 1.0001, float("nan"), None, "0.5"):
        with pytest.raises(ValueError, match="strength"):
            sampler.img2img_steps(10, bad)
    anc = _gd(50)
    for s, n in ((1e-6, 1), (0.5, 25), (1.0, 50)):
        plan, t0 = sampler._plan_img2img(anc, s)
        full = sampler._plan_ancestral(anc)
        assert len(plan.times) == n and t0 == n - 1 == full.times[50 - n]
        assert plan.times == full.times[50 - n:] and plan.rows == full.rows[50 - n:] and plan.draws == full.draws[50 - n:]
    ddim = _gd(1000, 10, ddim_sampling_eta=0.5)
    for s, n in ((1e-6, 1), (0.5, 5), (1.0, 10)):
        plan, t0 = sampler._plan_img2img(ddim, s)
        full = sampler._plan_ddim(ddim)
        assert (plan.times, plan.rows, plan.draws) == (full.times[10 - n:], full.rows[10 - n:], full.draws[10 - n:])
        assert t0 == full.times[10 - n] and plan.with_noise and plan.rederive and plan.clip
    dpm = _gd(1000, 10, sampler="dpm++")
    full = sampler._plan_dpm(dpm)
    for s, n in ((1e-6, 1), (0.5, 5), (1.0, 10)):
        plan, t0 = sampler._plan_img2img(dpm, s)
        pairs = dpm.dpm_time_pairs()[10 - n:]
        assert plan.times == full.times[10 - n:] and t0 == pairs[0][0] and plan.dpm
        assert plan.rows == tuple(sampler.dpm_coeffs(dpm, pairs, 2, False))
        assert plan.rows[0][6] == 0.0, "the first step of the truncated chain is first-order: no history is read"
        if 1 < n < 10:
            assert full.rows[10 - n][6] != 0.0 and plan.rows[1] == full.rows[10 - n + 1]
    assert sampler._plan_img2img(ddim, 0.5, kind="ancestral")[0].times == tuple(reversed(range(500)))
    with pytest.raises(ValueError, match="kind"):
        sampler._plan_img2img(ddim, 0.5, kind="euler")


def test_refusals_and_value_errors():
    img = torch.zeros(2, 3, 8, 8)
    sc = _gd(50, 5, net_kw=dict(self_condition=True))
    for call in (lambda: sc.encode(img), lambda: sc.decode(img), lambda: sc.reconstruct(img),
                 lambda: sc.interpolate(img, img, method="ddim")):
        with pytest.raises(NotImplementedError, match="self-conditioned"):
            call()
    lr = _gd(50, 5, net_kw=dict(lowres_cond=True), lowres_factor=2)
    for call in (lambda: lr.encode(img), lambda: lr.decode(img), lambda: lr.img2img(img),
                 lambda: lr.interpolate(img, img, method="ddim")):
        with pytest.raises(NotImplementedError, match="low-resolution"):
            call()
    gd = _gd(50, 5)
    for wrong in (torch.zeros(2, 3, 8, 4), torch.zeros(2, 1, 8, 8), torch.zeros(3, 8, 8), [0.0]):
        for call in (lambda: gd.encode(wrong), lambda: gd.decode(wrong), lambda: gd.img2img(wrong),
                     lambda: gd.interpolate(wrong, wrong, method="ddim")):
            with pytest.raises(ValueError, match="takes"):
                call()
    for s in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="strength"):
            gd.img2img(img, strength=s)
    for k in (0, 5, 9):
        with pytest.raises(ValueError, match="upto"):
            gd.encode(img, upto=k)
    for k in (-1, 5):
        with pytest.raises(ValueError, match="from_level"):
            gd.decode(img, from_level=k)
    with pytest.raises(ValueError, match="method"):
        gd.interpolate(img, img, method="slerp")
    with pytest.raises(ValueError, match="sampling_timesteps"):
        _gd(50).encode(img)                                       # no DDIM grid: steps must be given
    with pytest.raises(ValueError, match="steps"):
        gd.encode(img, steps=51)
    with pytest.raises(ValueError, match="cond_scale != 1"):
        gd.encode(img, classes=None, cond_scale=2.0) if gd.num_classes is not None else gd._guidance(None, 2.0, 2, "cpu")
    with pytest.raises(ValueError, match="noise must be"):
        gd.img2img(img, noise=torch.zeros(2, 3, 4, 4))


def test_ddpm_module_passes_through():
    from models.generative.diffusion.ddpm import DDPM, GaussianDiffusion
    for name in ("encode", "decode", "reconstruct", "img2img"):
        assert callable(getattr(DDPM, name)) and callable(getattr(GaussianDiffusion, name))
        assert "ema_model" in getattr(DDPM, name).__doc__ or "EMA" in getattr(DDPM, name).__doc__


def test_graph_keys():
    """every existing sampler configuration keeps its key (the enumeration of tests/test_sampler_trace_host.py::
    test_graph_keys, restated); the unclipped step has a key of its own, whatever the rest"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    S = (2, 3, 4, 4)
    net = Unet(dim=16, channels=3)
    mk = lambda objective, **kw: GaussianDiffusion(net, img_size=4, timesteps=6, objective=objective, **kw)  # noqa: E731
    v, eps = mk("pred_v"), mk("pred_noise")
    assert sampler._graph_key(v, S, True, False, False, False) == (S, True)
    assert sampler._graph_key(v, list(S), False, True, False, False) == (S, False)
    assert sampler._graph_key(eps, S, False, True, False, False) == (S, False, "pred_noise", True)
    assert sampler._graph_key(eps, S, False, True, True, False) == (S, False, "pred_noise", True, "guided")
    assert sampler._graph_key(eps, S, False, False, False, True) == ("dpm++", "pred_noise", S, False, "pred_noise", False)
    thr = mk("pred_v", dynamic_thresholding=True, dynamic_thresholding_percentile=0.995)
    assert sampler._graph_key(thr, S, True, False, False, True) == ("dynthresh", 0.995, "dpm++", "pred_v", S, True)
    assert sampler._graph_key(v, S, True, False, False, False, inpaint=True) == ("inpaint", S, True)
    assert sampler._graph_key(v, S, True, False, False, False, learned=True) == ("learned", S, True)
    seen = set()
    for gd in (v, eps, mk("pred_x0"), thr):
        for with_noise in (False, True):
            for rederive in (False, True):
                for guided in (False, True):
                    for dpm in (False, True):
                        for inpaint in (False, True):
                            args = (gd, S, with_noise, rederive, guided, dpm, inpaint)
                            base = sampler._graph_key(*args)
                            assert sampler._graph_key(*args, clip=True) == base and "noclip" not in base
                            assert sampler._graph_key(*args, clip=False) == ("noclip",) + base
                            seen.add(base)
    assert not any(k[0] == "noclip" for k in seen)
    # the inverse plan against the forward plan of the same diffusion and shape
    ddim = mk("pred_v", sampling_timesteps=3)
    fwd, inv = sampler._plan_ddim(ddim), sampler._plan_ddim_inverse(ddim)
    key = lambda p: sampler._graph_key(ddim, S, p.with_noise, p.rederive, False, p.dpm, clip=p.clip)  # noqa: E731
    assert key(fwd) == (S, False) and key(inv) == ("noclip", S, False) and key(inv) != key(fwd)
    assert key(sampler._plan_decode(ddim, clip=False)) == key(inv) and key(sampler._plan_decode(ddim)) == key(fwd)


def test_symbols_and_abi():
    from lgm_hip import _lib
    protos = _lib.parse_header()
    for name in ("lgm_slerp", "lgm_slerp_span", "lgm_slerp_partials"):
        assert name in protos
    assert len(protos["lgm_slerp"][1]) == 16 and protos["lgm_slerp_span"][1] == []
    assert _lib.ABI_VERSION == 8
    L = _lib.lib()
    assert L.lgm_abi_version() == 8
    span = int(L.lgm_slerp_span())
    assert span == 1024
    for B, HW in ((1, 1), (3, 64), (2, span), (2, span + 1), (1, 3 * span + 5), (8, 65536)):
        assert int(L.lgm_slerp_partials(B, HW)) == 3 * B * -(-HW // span)
    assert int(L.lgm_slerp_partials(0, 4)) < 0 and int(L.lgm_slerp_partials(4, 0)) < 0
    # the workgroup counts the design states: the chip's 256 CUs are covered at every benchmark shape, 8 x 8 is one workgroup
    assert [B * -(-HW // span) for B, HW in ((64, 64 * 64), (32, 128 * 128), (8, 256 * 256), (1, 64))] == [256, 512, 512, 1]


def test_slerp_reference_rule():
    """tests/edit_ref.py's slerp: the ends, the norm at the middle, the lerp branch"""
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((4, 3, 8, 8)), rng.standard_normal((4, 3, 8, 8))
    out, mag, c0, c1, lerp = edit_ref.slerp(a, b, [0.0, 1.0, 0.5, 0.3])
    assert not lerp.any() and np.array_equal(out[0], a[0]) and np.abs(out[1] - b[1]).max() < 1e-15
    assert (c0[0], c1[0]) == (1.0, 0.0) and c0[1] == 0.0 and abs(c1[1] - 1.0) < 1e-15
    na, nb, nm = (np.sqrt((x[2] ** 2).sum()) for x in (a, b, out))
    assert abs(nm - 0.5 * (na + nb)) < 0.02 * nm                  # a lerp of two independent Gaussians has norm ~ 0.71 of that
    assert (mag >= np.abs(out) - 1e-12).all()
    for bb in (a, a * (1 + 1e-4), -a):
        _, _, c0, c1, lerp = edit_ref.slerp(a, bb, [0.25] * 4)
        assert lerp.all() and np.allclose(c0, 0.75) and np.allclose(c1, 0.25)
    _, _, c0, c1, lerp = edit_ref.slerp(np.zeros_like(a), b, [0.25] * 4)
    assert lerp.all() and np.allclose(c0, 0.75)


def test_fixture(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "diffusion_edit.npz")))
    B, S = int(fx["B"]), int(fx["S"])
    assert (int(fx["dim"]), S, B, int(fx["T"]), int(fx["T_anc"])) == (16, 8, 4, 1000, 50)
    assert fx["img"].shape == fx["q_noise"].shape == (B, 3, S, S) and fx["anc_noises"].shape == (25, B, 3, S, S)
    for o in ("pred_v", "pred_noise"):
        for case in ("enc10", "enc20", "dec10", "dec20", "genc", "i2i_anc", "i2i_ddim", "i2i_dpm", "interp", "interp:za",
                     "interp:zb"):
            a, e = fx[f"{o}:{case}"], fx[f"{o}:{case}64"]
            assert a.shape == e.shape == (B, 3, S, S) and a.dtype == np.float32 and e.dtype == np.float64, (o, case)
            assert np.isfinite(a).all() and np.isfinite(e).all()
            assert np.linalg.norm(a - e) <= 1e-2 * np.linalg.norm(e), (o, case)
        assert fx[f"{o}:interp:mix"].shape == (B, 3, S, S) and fx[f"{o}:interp:coef64"].shape == (B, 2)
        for name in ("10", "20"):
            steps, upto = (int(v) for v in fx[f"grid:{o}:{name}"])
            assert (upto if upto > 0 else steps - 1) == int(name), "the inversion has as many pairs as its name says"
            err, apart = fx[f"roundtrip:{o}:{name}"]
            assert err < 0.25 * apart, "the tool's own float64 round trip reconstructs"


@pytest.mark.parametrize("kind", ["ancestral", "ddim_eta0", "ddim_eta1", "dpm_ode", "dpm_sde"])
def test_existing_samplers_issue_the_launches_they_issued(monkeypatch, kind):
    """``sample()`` on the three samplers under the recorder of tests/test_sampler_trace_host.py (read, not modified): first
    that file's own check of the whole chain - every entry point, scalar and pointer role it pins, the clip flag among them -
    on this tree, then the entry points ``sample()`` issues against that pinned sequence."""
    import test_sampler_trace_host as TH
    ses = TH._Session(monkeypatch)
    TH._run_and_check(ses, kind, "pred_v", False, False)
    pinned = [name for name, _ in ses.rec.calls]
    assert pinned and pinned[0] == "lgm_nchw_to_nhwc" and pinned[-1] == "lgm_nhwc_to_nchw"
    again = TH._Session(monkeypatch)
    gd = again.diffusion(kind, "pred_v", False, False)
    out = gd.sample(batch_size=TH.B)
    assert tuple(out.shape) == TH.SHAPE
    assert [name for name, _ in again.rec.calls] == pinned
    assert not any("slerp" in name for name in pinned)
