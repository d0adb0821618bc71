"""CPU: the variational-bound likelihood (bits per dimension) at the layers that need no GPU - the row plan of
lgm_hip.likelihood against float64 closed forms written out here, numpy restatements of the decoder term (the kernel's
cancellation-free float32 form holds 1e-5 per element where the textbook float32 form misses 1e-4 per sample), the C-ABI, the
graph key, ``nll_bpd`` / ``DDPM.bits_per_dim`` / ``DDPM.bpd_every`` and tests/golden/diffusion_bpd.npz's own consistency."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def gd():
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    return GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)     # sigmoid schedule


def f32(x):
    return float(np.float32(x))


def closed_forms(gd):
    """float64 from the diffusion's tables, written from the formulas: lv_q, both lv_p conventions"""
    betas = gd.betas.double().numpy()
    lv_q = gd.posterior_log_variance_clipped.double().numpy()
    small = np.concatenate([lv_q[1:2], lv_q[1:]])
    large = np.concatenate([lv_q[1:2], np.log(betas[1:])])
    return betas, gd.alphas_cumprod.double().numpy(), lv_q, {"fixed_small": small, "fixed_large": large}


def test_plan_rows_match_float64_closed_forms(gd):
    from lgm_hip import likelihood as LK
    T = gd.num_timesteps
    betas, acp, lv_q, lv_p = closed_forms(gd)
    assert lv_q[0] == pytest.approx(math.log(1e-20)), "the reference's clipped table: not the model's variance at t = 0"
    for variance in LK.VARIANCES:
        rows = LK.vlb_plan(gd, None, variance)
        assert len(rows) == T + 1 and all(len(r) == LK.VLB_ROW for r in rows)
        assert [int(r[6]) for r in rows] == [LK.KL] * (T - 1) + [LK.DECODER, LK.PRIOR]
        for row, t in zip(rows, reversed(range(T))):
            assert all(f32(c) == c for c in row), "every scalar is a float32 value"
            want_head = (gd.sqrt_alphas_cumprod[t], gd.sqrt_one_minus_alphas_cumprod[t], gd.sqrt_recip_alphas_cumprod[t],
                         gd.sqrt_recipm1_alphas_cumprod[t], gd.posterior_mean_coef1[t], gd.posterior_mean_coef2[t])
            assert row[:6] == tuple(float(v) for v in want_head), t
            lp = lv_p[variance][t]
            assert row[10] == f32(lp) and row[11] == f32(lv_q[t])
            if t == 0:
                assert row[7:10] == (0.0, 0.0, f32(math.exp(-0.5 * lp)))
            else:
                kc = 0.5 * (-1.0 + lp - lv_q[t] + math.exp(lv_q[t] - lp))
                # KC cancels to ~d^2 / 4 at small d = lv_q - lv_p: this form keeps ~1e-16 absolute, the plan's expm1 more
                assert abs(row[7] - kc) <= 1e-6 * kc + 1e-15 and row[8] == f32(0.5 * math.exp(-lp)) and row[9] == 0.0
                if variance == "fixed_small":
                    assert row[7] == 0.0, "fixed_small: the two variances are the same number"
                elif t < T - 1:
                    assert row[7] > 0.0, t
        # both conventions at t = 0 and t = 1: log beta~_1 at t = 0, and sigma there is of the order of the bin
        r0, r1 = rows[T - 1], rows[T - 2]
        assert r0[10] == f32(lv_q[1]) and r1[10] == (f32(lv_q[1]) if variance == "fixed_small" else f32(math.log(betas[1])))
        assert 0.005 < 1.0 / r0[9] < 0.05
        # the prior row
        a = acp[-1]
        pr = rows[-1]
        assert pr[:6] == (0.0,) * 6 and pr[10] == f32(a) and pr[11] == f32(math.log1p(-a))
        assert pr[7] == f32(0.5 * (-1.0 - math.log1p(-a) + (1.0 - a))) and pr[8] == f32(0.5 * a) and pr[7] > 0.0
    assert LK.vlb_plan(gd) == LK.vlb_plan(gd, list(reversed(range(T))), "fixed_small"), "the defaults"


def test_plan_keeps_the_order_given_and_rejects_bad_arguments(gd):
    from lgm_hip import likelihood as LK
    full = {t: r for t, r in zip(reversed(range(1000)), LK.vlb_plan(gd, None, "fixed_large"))}
    ts = [0, 999, 3, 500]
    rows = LK.vlb_plan(gd, ts, "fixed_large")
    assert len(rows) == 5 and rows[:4] == [full[t] for t in ts] and int(rows[0][6]) == LK.DECODER and int(rows[4][6]) == LK.PRIOR
    assert len(LK.vlb_plan(gd, [])) == 1
    for bad in ([1000], [-1], [5, 1000]):
        with pytest.raises(ValueError, match="timesteps"):
            LK.vlb_plan(gd, bad)
    with pytest.raises(ValueError, match="distinct"):
        LK.vlb_plan(gd, [5, 7, 5])
    with pytest.raises(ValueError, match="variance"):
        LK.vlb_plan(gd, None, "learned")


# ----------------------------------------------------------------------------------------------------------------------
# the decoder term: numpy restatements on crafted inputs
# ----------------------------------------------------------------------------------------------------------------------
LOG_SIGMAS = (-4.4, -3.0, -1.0, 0.0)
FIXED_Z = (0.0, 4.6, 5.5, 6.1, -6.1, 7.5)


def crafted_decoder_inputs(n_per=75, samples=4, seed=0):
    """-> (x, mean, inv_std) float32 [len(LOG_SIGMAS) * samples, n_per]: images on the 8-bit grid with exactly +-1 and +-(1 -
    2/255) among them, standardised residuals uniform in [-9, 9] plus FIXED_Z, one log sigma per block of ``samples`` rows"""
    rng = np.random.default_rng(seed)
    xs, means, invs = [], [], []
    for ls in LOG_SIGMAS:
        sigma = math.exp(ls)
        for _ in range(samples):
            x = rng.integers(0, 256, n_per) / 255.0 * 2.0 - 1.0
            x[:4] = (-1.0, 1.0, -(1.0 - 2.0 / 255.0), 1.0 - 2.0 / 255.0)
            z = rng.uniform(-9.0, 9.0, n_per)
            z[4:4 + len(FIXED_Z)] = FIXED_Z
            xs.append(x.astype(np.float32))
            means.append((x - z * sigma).astype(np.float32))
            invs.append(np.full(n_per, np.float32(1.0 / sigma)))
    return np.stack(xs), np.stack(means), np.stack(invs).astype(np.float32)


def decoder_canonical(x, mean, inv_std, dtype):
    """Nichol & Dhariwal's discretized_gaussian_log_likelihood, the textbook form, evaluated in ``dtype``"""
    x, mean, inv_std = (a.astype(dtype) for a in (x, mean, inv_std))
    one, half = dtype(1.0), dtype(0.5)
    cdf = lambda z: half * (one + np.tanh(dtype(math.sqrt(2.0 / math.pi)) * (z + dtype(0.044715) * z ** 3)))  # noqa: E731
    c = x - mean
    plus, minus = cdf(inv_std * (c + dtype(1.0 / 255.0))), cdf(inv_std * (c - dtype(1.0 / 255.0)))
    floor = dtype(1e-12)
    lp = np.log(np.maximum(plus, floor))
    lm = np.log(np.maximum(one - minus, floor))
    ld = np.log(np.maximum(plus - minus, floor))
    return np.where(x < dtype(-0.999), lp, np.where(x > dtype(0.999), lm, ld))


def decoder_stable32(x, mean, inv_std):
    """the kernel's form (csrc/elementwise.hip vlb_decoder_logp), every operation in float32"""
    F = np.float32
    K, C3, FLOOR = F(0.7978845608), F(0.044715), F(-27.6310211)
    zc, dl = inv_std * (x - mean), inv_std * F(1.0 / 255.0)
    softplus = lambda v: np.where(v > 0, v + np.log1p(np.exp(-np.abs(v))), np.log1p(np.exp(-np.abs(v))))  # noqa: E731
    z = np.where(x < 0, zc + dl, zc - dl)
    a = F(2.0) * (K * (z + C3 * (z * z * z)))
    edge = -softplus(np.where(x < 0, -a, a)).astype(F)
    h = K * (F(2.0) * dl + C3 * (F(6.0) * (zc * zc) * dl + F(2.0) * (dl * dl * dl)))
    m = np.abs(K * (F(2.0) * zc + C3 * (F(2.0) * (zc * zc * zc) + F(6.0) * zc * (dl * dl))))
    big = np.maximum(h, m)
    rest = np.where(h >= m, np.exp(m - h) + np.exp(-m - h) + np.exp(-F(2.0) * h), np.exp(h - m) + np.exp(-h - m) + np.exp(-F(2.0) * m))
    y = F(2.0) * h
    log1mexp = np.where(y > F(0.69314718), np.log1p(-np.exp(-y)), np.log(-np.expm1(-y)))
    mid = (h - big) + log1mexp - np.log1p(rest)
    out = np.where((x < F(-0.999)) | (x > F(0.999)), edge, mid)
    assert out.dtype == np.float32
    return np.maximum(out, FLOOR)


def test_the_stable_float32_decoder_form_holds_where_the_textbook_form_fails():
    x, mean, inv_std = crafted_decoder_inputs()
    want = decoder_canonical(x, mean, inv_std, np.float64)
    assert np.isfinite(want).all() and (want <= 0).all()
    z = inv_std.astype(np.float64) * (x.astype(np.float64) - mean)
    assert z.min() < -8 and z.max() > 8 and (want == want.min()).sum() > 10, "the floor is reached"
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        stable = decoder_stable32(x, mean, inv_std).astype(np.float64)
        naive = decoder_canonical(x, mean, inv_std, np.float32).astype(np.float64)
    # an edge element far inside its bin has p == 1 in float64 (log p == 0): there the stable form's -e^{-a} is held to 1e-15
    per_elem = np.abs(stable - want) / np.maximum(np.abs(want), 1e-10)
    per_sample = lambda a: np.abs(a.mean(1) - want.mean(1)) / np.abs(want.mean(1))  # noqa: E731
    print(f"stable float32: {per_elem.max():.3e} per element, {per_sample(stable).max():.3e} per sample; "
          f"textbook float32: {per_sample(naive).max():.3e} per sample")
    assert per_elem.max() <= 1e-5
    assert per_sample(stable).max() <= 1e-6
    assert per_sample(naive).max() > 1e-4, "the inputs no longer tell the two forms apart"


# ----------------------------------------------------------------------------------------------------------------------
# library and API
# ----------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported():
    from lgm_hip import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lgm_vlb_term", "lgm_vlb_term_table"):
        assert name in protos, f"{name} is not declared in include/lgm_hip.h"
        assert hasattr(dll, name), f"{name} is not exported by the library"
    assert len(protos["lgm_vlb_term"][1]) == 27 and len(protos["lgm_vlb_term_table"][1]) == 20
    L = _lib.lib()
    assert L.lgm_abi_version() == _lib.ABI_VERSION == 8
    syms = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "vlb_term_kernel(" in syms, "the library holds no vlb_term_kernel"
    names = [L.lgm_kernel_name(i) for i in range(L.lgm_kernel_name_count())]
    assert not any(b"vlb_term" in (n or b"") for n in names), "the name is noted without a registry entry"
    # the host rejects bad arguments before any launch (no GPU needed)
    buf = (ctypes.c_float * 512)()
    p = ctypes.addressof(buf)
    img, nz, xin, v, out, tab = p, p + 256, p + 512, p + 768, p + 1024, p + 1280
    ok = dict(img=img, noise=nz, xin=xin, pitch=4, x_off=0, v=v, v_pitch=4, B=1, C=3, HW=1, objective=2, kind=0, out=out,
              n_rows=2, out_row=0)

    def term(**kw):
        a = dict(ok, **kw)
        L.lgm_vlb_term(a["img"], a["noise"], 1, a["xin"], a["pitch"], a["x_off"], a["v"], a["v_pitch"], a["B"], a["C"],
                       a["HW"], a["objective"], 1, 0.5, 0.5, 2.0, 1.0, 0.1, 0.9, a["kind"], 0.0, 1.0, 1.0, a["out"],
                       a["n_rows"], a["out_row"], None)
    for kw in (dict(img=None), dict(noise=None), dict(xin=None), dict(v=None), dict(out=None), dict(out=img), dict(out=xin),
               dict(objective=3), dict(kind=3), dict(kind=-1), dict(out_row=2), dict(out_row=-1), dict(n_rows=0), dict(B=0),
               dict(x_off=2), dict(v_pitch=2), dict(C=5), dict(kind=2, img=None)):
        with pytest.raises(_lib.LgmArgumentError, match="vlb_term"):
            term(**kw)

    def table(**kw):
        a = dict(dict(ok, table=tab, stride=12, counter=p + 1400), **kw)
        L.lgm_vlb_term_table(a["img"], a["noise"], 1, a["xin"], a["pitch"], a["x_off"], a["v"], a["v_pitch"], a["B"], a["C"],
                             a["HW"], a["objective"], 1, a["table"], a["stride"], a["counter"], a["out"], a["n_rows"], 1, None)
    for kw in (dict(table=None), dict(counter=None), dict(stride=8), dict(noise=None), dict(out=tab), dict(n_rows=0)):
        with pytest.raises(_lib.LgmArgumentError, match="vlb_term_table"):
            table(**kw)


def test_graph_key_can_never_be_a_samplers(gd):
    from lgm_hip import likelihood as LK, sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    shape = (4, 3, 16, 16)
    key = LK._vlb_key(gd, shape, True)
    assert key[:3] == ("vlb", "pred_v", True) and LK._vlb_key(gd, shape, False)[:3] == ("vlb", "pred_v", False)
    assert key != LK._vlb_key(gd, shape, False) and key != LK._vlb_key(gd, (2, 3, 16, 16), True)
    net = Unet(dim=16, channels=3)
    firsts = set()
    for objective in ("pred_v", "pred_noise", "pred_x0"):
        for dyn in (False, True):
            g = GaussianDiffusion(net, img_size=16, objective=objective, dynamic_thresholding=dyn)
            assert LK._vlb_key(g, shape, True)[:3] == ("vlb", objective, True)
            for wn in (False, True):
                for red in (False, True):
                    for guided in (False, True):
                        for dpm in (False, True):
                            for inp in (False, True):
                                k = sampler._graph_key(g, shape, wn, red, guided, dpm, inp)
                                firsts.add(k[0])
                                assert k != LK._vlb_key(g, shape, True) and k != LK._vlb_key(g, shape, False)
    assert "vlb" not in firsts and firsts == {shape, "dpm++", "dynthresh", "inpaint"}


def test_nll_bpd_rejects_a_subset(gd):
    with pytest.raises(ValueError, match="subset"):
        gd.nll_bpd(torch.zeros(1, 3, 16, 16), timesteps=[999, 0])
    with pytest.raises(ValueError, match="img must be"):
        gd.vlb_terms(torch.zeros(1, 3, 8, 8), timesteps=[0])


def test_ddpm_bits_per_dim_and_bpd_every():
    import inspect
    from models.generative.diffusion.ddpm import DDPM
    names = list(inspect.signature(DDPM.__init__).parameters)
    assert "bpd_every" not in names and names[-4:] == ["cond_scale", "sampler", "dpm_order", "dpm_stochastic"]
    m = DDPM(img_size=16, dim=16)
    assert m.bpd_every == 0 and m.sample_every == 1000 and "bpd_every" not in m.hparams
    m.sample_every = 0
    m.eval()
    ema = m.ema.ema_model
    logs, calls = [], []
    m.log = lambda name, value, **kw: logs.append((name, float(value)))
    ema.forward = lambda data, **kw: torch.tensor(0.25)

    def nll(img, **kw):
        calls.append((tuple(img.shape), kw, ema.training))
        return torch.tensor([1.0, 3.0], dtype=torch.float64)
    ema.nll_bpd = nll
    batch = (torch.rand(2, 3, 16, 16), torch.zeros(2, dtype=torch.long))
    for _ in range(3):
        assert float(m.validation_step(batch)) == 0.25
    assert logs == [("val_loss", 0.25)] * 3 and not calls, "bpd_every = 0: what validation_step logged before, nothing more"
    # bits_per_dim: the EMA diffusion in eval mode, arguments passed through
    ema.train()
    out = m.bits_per_dim(batch[0], variance="fixed_large")
    assert out.tolist() == [1.0, 3.0] and calls == [((2, 3, 16, 16), dict(classes=None, variance="fixed_large"), False)]
    # every second validation batch
    del logs[:], calls[:]
    m.bpd_every = 2
    for _ in range(5):
        m.validation_step(batch)
    assert [n for n, _ in logs] == ["val_loss", "val_bpd", "val_loss", "val_loss", "val_bpd", "val_loss", "val_loss", "val_bpd"]
    assert all(v == 2.0 for n, v in logs if n == "val_bpd") and len(calls) == 3
    assert all(kw == dict(classes=None) for _, kw, _ in calls), "a network without classes is not handed the batch's labels"


def test_fixture_is_self_consistent(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "diffusion_bpd.npz")))
    assert int(fx["T"]) == 1000 and int(fx["short_T"]) == 20 and int(fx["B"]) == 4
    assert tuple(fx["times"]) == (999, 998, 750, 500, 250, 2, 1, 0) and tuple(fx["classes"]) == (3, 0, 3, 5)
    img = fx["img"]
    assert img.shape == (4, 3, 16, 16) and np.array_equal(np.round(img * 255) / 255, img.astype(np.float64).astype(np.float32))
    cases = ["pred_v:small", "pred_v:large", "pred_noise:small", "pred_noise:large", "pred_v:noclip", "pred_v:selfcond",
             "pred_v:labels"]
    for case in cases:
        for steps, n in ((1000, 8), (20, 20)):
            for k in ("vb", "xstart_mse", "mse"):
                a, a64 = fx[f"{case}:{steps}:{k}"], fx[f"{case}:{steps}:{k}64"]
                assert a.dtype == np.float32 and a64.dtype == np.float64 and a.shape == a64.shape == (n, 4)
                assert np.isfinite(a64).all() and (a64 >= 0).all()
            vb, vb64 = fx[f"{case}:{steps}:vb"], fx[f"{case}:{steps}:vb64"]
            assert (np.abs(vb[:-1] - vb64[:-1]) / vb64[:-1]).max() <= 1e-3, "KL terms: float32 against float64"
            assert fx[f"{case}:{steps}:prior64"].shape == (4,)
        total = fx[f"{case}:20:total64"]
        assert np.allclose(total, fx[f"{case}:20:vb64"].sum(0) + fx[f"{case}:20:prior64"], rtol=1e-14, atol=0)
        assert (total > 1.0).all() and (total < 40.0).all()
    assert not np.array_equal(fx["pred_v:small:20:vb"], fx["pred_v:large:20:vb"])
    assert not np.array_equal(fx["pred_v:small:20:vb"], fx["pred_v:selfcond:20:vb"])
    assert not np.array_equal(fx["pred_v:small:20:vb"], fx["pred_v:labels:20:vb"])
    assert not np.array_equal(fx["pred_v:small:20:vb"], fx["pred_v:noclip:20:vb"])
