"""GPU: DDIM inversion (``encode``), ``decode``, ``img2img`` and the slerp interpolation (extensions of the reference).

  * csrc/slerp.hip per element against the float64 rule of tests/edit_ref.py: the roundings of an output element on the way
    from the per-sample sums are c0 (or c1) to float32, the product c0 a, the fma - three - each at most u
    relative to a partial result bounded by |c0 a| + |c1 b|; the sums themselves are double (n 2^-53 relative) and reach an
    element through (c0, c1), asserted within 2 u of float64 on their own: the bound is (3 + 2) u (|c0 a| + |c1 b|);
  * two runs and a run under another CU margin give equal bits;
  * the chains against tests/golden/diffusion_edit.npz (tools/make_golden_edit.py: loops around the REFERENCE's network and
    model_predictions): 1e-4 relative; where the reference's own float32 result stands further than 1e-5 from the fixture's
    float64 evaluation, HIP is held to float64 instead, no further than three times the reference's own distance;
  * graph replay against eager launches, bit for bit; the default ``interpolate`` against the calls it has always made.

Measured distances go through the ``parity`` recorder (committed record: profiles/r20_edit_parity.json).
"""
import os

import numpy as np
import pytest
import torch

import edit_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = 2.0 ** -24
ROUNDINGS = 3
SENTINEL = 7.0


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _r4(n):
    return (n + 3) // 4 * 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_edit.npz")))


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------
def _span():
    from lgm_hip import ops
    return ops.slerp_span()


SHAPES = {"one_partial_span": lambda S: (3, 3, 64), "exactly_one_span": lambda S: (2, 1, S),
          "two_spans": lambda S: (2, 3, S + 1), "several_spans": lambda S: (1, 3, 3 * S + 5)}
# (pitch, offset) from C: the 16-byte form; the same slice behind another (still 16-byte); lanes no 16-byte access can take
LAYOUTS = {"dense": lambda C: (_r4(C), 0), "second_slice": lambda C: (2 * _r4(C), _r4(C)),
           "odd_lanes": lambda C: (2 * _r4(C) + 1, 1)}
LAMS = ([0.0, 1.0, 0.5], [0.3, 0.5, 1.0])


def _operand(values, pitch, off, dev):
    """values [B, HW, C] in lanes [off, off + C) of a sentinel-filled [B, 1, HW, pitch] buffer -> (buffer, view of the lanes)"""
    B, HW, C = values.shape
    buf = torch.full((B, 1, HW, pitch), SENTINEL)
    buf[:, 0, :, off:off + C] = values
    buf = buf.to(dev)
    return buf, buf[..., off:off + C]


def _check_slerp(dev, a, b, lam, pitch, off, what, expect_lerp=None, in_place=False):
    from lgm_hip import ops
    B, HW, C = a.shape
    abuf, av = _operand(a, pitch, off, dev)
    bbuf, bv = _operand(b, pitch, off, dev)
    obuf, ov = (abuf, av) if in_place else _operand(torch.full_like(a, SENTINEL), pitch, off, dev)
    coef = torch.full((B, 2), SENTINEL, device=dev)
    lam_t = torch.tensor(lam, dtype=torch.float32, device=dev)
    ret = ops.slerp(av, bv, lam_t, out=ov, coef_out=coef)
    assert ret is ov and ops.lib()._dll.lgm_last_kernel().decode() == "slerp_blend_kernel"
    want, mag, c0, c1, lerp = edit_ref.slerp(a.numpy(), b.numpy(), lam)
    if expect_lerp is not None:
        assert lerp.tolist() == [expect_lerp] * B, what
    _, _, _, c = edit_ref.slerp_cosine(a.numpy(), b.numpy())
    for i in np.nonzero(~lerp)[0]:                                # the reference alone decides the branch
        assert abs((1.0 - c[i] * c[i]) - edit_ref.LERP_SWITCH) > 1e-4, (what, i)
    got = obuf.cpu()[:, 0]
    live = got[..., off:off + C].double().numpy()
    bound = (ROUNDINGS + 2) * U * mag
    err = np.abs(live - want) - bound
    print(f"[slerp] {what}: worst error over its bound {float((np.abs(live - want) / np.maximum(bound, 1e-300)).max()):.3f}")
    assert float(err.max()) <= 0.0, what
    k = coef.cpu().double().numpy()
    for got_c, ref_c in ((k[:, 0], c0), (k[:, 1], c1)):
        assert (np.abs(got_c - ref_c) <= 2 * U * np.abs(ref_c)).all(), (what, got_c, ref_c)
    for i, l in enumerate(lam):                                   # the ends return an operand to the bit
        if l == 0.0:
            assert torch.equal(got[i, :, off:off + C], a[i]), what
        if l == 1.0:
            assert torch.equal(got[i, :, off:off + C], b[i]), what
    untouched = torch.ones(pitch, dtype=torch.bool)
    untouched[off:off + C] = False
    if untouched.any():
        assert bool((got[..., untouched] == SENTINEL).all()), f"{what}: a lane outside the slice was written"
    if not in_place:
        ah, _ = _operand(a, pitch, off, torch.device("cpu"))
        assert torch.equal(abuf.cpu(), ah), "a is read only"
    bh, _ = _operand(b, pitch, off, torch.device("cpu"))
    assert torch.equal(bbuf.cpu(), bh), "b is read only"
    return got


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_slerp_kernel_against_float64(dev, shape, layout):
    B, C, HW = SHAPES[shape](_span())
    pitch, off = LAYOUTS[layout](C)
    g = torch.Generator().manual_seed(10 * list(SHAPES).index(shape) + list(LAYOUTS).index(layout))
    for n, lams in enumerate(LAMS):
        a, b = torch.randn(B, HW, C, generator=g), torch.randn(B, HW, C, generator=g)
        _check_slerp(dev, a, b, lams[:B], pitch, off, f"{shape}/{layout}/lams{n}", expect_lerp=False)
    _check_slerp(dev, a, b, LAMS[1][:B], pitch, off, f"{shape}/{layout}/in place", expect_lerp=False, in_place=True)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_slerp_kernel_lerp_branch(dev, layout):
    B, C, HW = 3, 3, 64
    pitch, off = LAYOUTS[layout](C)
    a = torch.randn(B, HW, C, generator=torch.Generator().manual_seed(3))
    other = torch.randn(B, HW, C, generator=torch.Generator().manual_seed(4))
    lam = [0.3, 0.5, 1.0]
    for name, (x, y) in {"b = a": (a, a.clone()), "b = (1 + 1e-4) a": (a, a * (1 + 1e-4)), "a = 0": (torch.zeros_like(a), other),
                         "b = 0": (a, torch.zeros_like(a)), "b = -a": (a, -a)}.items():
        _check_slerp(dev, x, y, lam, pitch, off, f"lerp branch, {name}, {layout}", expect_lerp=True)


def test_slerp_forms_agree_and_runs_repeat(dev):
    """The 16-byte form and the one-float form visit the same elements in the same order: equal bits.  Two runs give equal
    bits (no atomics), and so does a run under another CU margin (the span does not depend on it)."""
    from lgm_hip import ops
    S = _span()
    B, C, HW = 2, 3, 2 * S + 77
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(B, HW, C, generator=g), torch.randn(B, HW, C, generator=g)
    lam = torch.tensor([0.3, 0.7], device=dev)

    def run(layout):
        pitch, off = LAYOUTS[layout](C)
        _, av = _operand(a, pitch, off, dev)
        _, bv = _operand(b, pitch, off, dev)
        coef = torch.zeros(B, 2, device=dev)
        return ops.slerp(av, bv, lam, coef_out=coef).clone(), coef
    first, k1 = run("dense")
    again, k2 = run("dense")
    assert torch.equal(first, again) and torch.equal(k1, k2)
    for layout in ("second_slice", "odd_lanes"):
        other, k = run(layout)
        assert torch.equal(first, other) and torch.equal(k1, k), layout
    L = ops.lib()
    before = L.lgm_cu_margin()
    try:
        L.lgm_set_cu_margin(16)
        assert ops.slerp_span() == S and ops.slerp_partials(B, HW) == 3 * B * 3
        margin, k = run("dense")
    finally:
        L.lgm_set_cu_margin(before)
    assert torch.equal(first, margin) and torch.equal(k1, k)


# ----------------------------------------------------------------------------------------------------------------------
# chains against the reference fixture
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(fx, dev):
    from models.generative.diffusion.ddpm import Unet
    from oracle import diffusion as OD
    P = OD.unet_init(dim=int(fx["dim"]), channels=3, seed=int(fx["seed"]))
    plain = Unet(dim=int(fx["dim"]), channels=3)
    plain.load_state_dict(P, strict=True)
    guided = Unet(dim=int(fx["dim"]), channels=3, num_classes=int(fx["K"]))
    guided.load_state_dict(dict(P, **{"label_emb.weight": torch.as_tensor(fx["label_emb.weight"])}), strict=True)
    return {"plain": plain, "guided": guided}


def _diffusion(net, dev, fx, objective, T=None, **kw):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    gd = GaussianDiffusion(net, img_size=int(fx["S"]), timesteps=int(fx["T"]) if T is None else T, objective=objective, **kw).to(dev)
    net.prepare_hip(dev)
    return gd


def _arbiter(parity, what, hip, ref, exact):
    """1e-4 against the reference's float32 result, unless that result itself stands further than 1e-5 from the float64
    evaluation of the same inputs: then HIP is held to float64, no further from it than three times the reference is."""
    e, d_ref, d_hip = rel(hip, ref), rel(ref, exact), rel(hip, exact)
    parity.record(what + " [distances to float64]", hip_vs_ref=e, ref_vs_fp64=d_ref, hip_vs_fp64=d_hip)
    print(f"[parity] {what}: |hip-ref| {e:.3e}; distance to float64: reference {d_ref:.3e}, hip {d_hip:.3e}")
    if d_ref <= 1e-5:
        return parity(what, e, RTOL)
    assert d_hip <= 3 * d_ref, (what, e, d_hip, d_ref)


def _grid(fx, o, name):
    steps, upto = (int(v) for v in fx[f"grid:{o}:{name}"])
    return steps, (upto if upto > 0 else None)


@pytest.mark.parametrize("objective", ["pred_v", "pred_noise"])
def test_inversion_and_decode_match_reference_fixture(fx, nets, dev, parity, objective):
    o = objective
    gd = _diffusion(nets["plain"], dev, fx, o, sampling_timesteps=10)
    img = torch.as_tensor(fx["img"]).to(dev)
    for name in ("10", "20"):
        steps, upto = _grid(fx, o, name)
        z = gd.encode(img, steps=steps, upto=upto)
        assert z.shape == img.shape and torch.isfinite(z).all()
        _arbiter(parity, f"{o}: {name}-pair inversion, latent", z, fx[f"{o}:enc{name}"], fx[f"{o}:enc{name}64"])
        back = gd.decode(torch.as_tensor(fx[f"{o}:enc{name}"]).to(dev), from_level=upto, steps=steps, clip=False)
        _arbiter(parity, f"{o}: decode of the {name}-pair latent", back, fx[f"{o}:dec{name}"], fx[f"{o}:dec{name}64"])
        # the round trip on HIP's own latent reconstructs as the tool's float64 one does
        mine = gd.reconstruct(img, steps=steps, upto=upto)
        err = float((mine - img).double().pow(2).mean().sqrt())
        tool_err, apart = (float(v) for v in fx[f"roundtrip:{o}:{name}"])
        parity.record(f"{o}: {name}-pair round trip RMS", hip=err, tool_fp64=tool_err, images_apart=apart)
        assert err < 0.25 * apart
    # guided, class-conditional
    cg = _diffusion(nets["guided"], dev, fx, o, sampling_timesteps=10)
    steps, upto = _grid(fx, o, "10")
    y = torch.as_tensor(fx["classes"]).to(dev)
    z = cg.encode(img, steps=steps, upto=upto, classes=y, cond_scale=float(fx["cond_scale"]))
    _arbiter(parity, f"{o}: guided 10-pair inversion, latent", z, fx[f"{o}:genc"], fx[f"{o}:genc64"])
    assert not torch.equal(z, cg.encode(img, steps=steps, upto=upto, classes=y, cond_scale=1.0))


@pytest.mark.parametrize("objective", ["pred_v", "pred_noise"])
def test_img2img_matches_reference_fixture(fx, nets, dev, parity, objective):
    from lgm_hip import sampler
    o, net = objective, nets["plain"]
    img = torch.as_tensor(fx["img"]).to(dev)
    qn = torch.as_tensor(fx["q_noise"]).to(dev)
    strength, n = float(fx["strength"]), int(fx["i2i_steps"])
    anc = _diffusion(net, dev, fx, o, T=int(fx["T_anc"]))
    noises = [x.to(dev) for x in torch.as_tensor(fx["anc_noises"])]
    out = sampler.img2img(anc, anc.normalize(img), strength, qn, noises=noises)
    _arbiter(parity, f"{o}: img2img, ancestral chain of 25 of 50", out, fx[f"{o}:i2i_anc"], fx[f"{o}:i2i_anc64"])
    ddim = _diffusion(net, dev, fx, o, sampling_timesteps=n)
    _arbiter(parity, f"{o}: img2img, DDIM 5 of 10", ddim.img2img(img, strength, noise=qn), fx[f"{o}:i2i_ddim"],
             fx[f"{o}:i2i_ddim64"])
    dpm = _diffusion(net, dev, fx, o, sampling_timesteps=n, sampler="dpm++")
    _arbiter(parity, f"{o}: img2img, DPM-Solver++ 5 of 10", dpm.img2img(img, strength, noise=qn), fx[f"{o}:i2i_dpm"],
             fx[f"{o}:i2i_dpm64"])
    # strength 1 on the DDIM grid is the whole sampler from q_sample at its first time
    full = ddim.img2img(img, 1.0, noise=qn)
    tb = torch.full((img.shape[0],), ddim.ddim_time_pairs()[0][0], device=dev, dtype=torch.long)
    assert torch.equal(full, sampler.ddim_sample(ddim, tuple(img.shape), init_noise=ddim.q_sample(ddim.normalize(img), tb, qn)))


@pytest.mark.parametrize("objective", ["pred_v", "pred_noise"])
def test_ddim_interpolation_matches_reference_fixture(fx, nets, dev, parity, objective):
    from lgm_hip import ops
    o = objective
    gd = _diffusion(nets["plain"], dev, fx, o, sampling_timesteps=10)
    steps, upto = _grid(fx, o, "10")
    x1 = torch.as_tensor(fx["img"]).to(dev) * 2 - 1
    x2 = x1.roll(1, 0)
    out = gd.interpolate(x1, x2, lam=float(fx["lam"]), method="ddim", steps=steps, upto=upto)
    _arbiter(parity, f"{o}: DDIM interpolation at lam 0.5", out, fx[f"{o}:interp"], fx[f"{o}:interp64"])
    per = gd.interpolate(x1, x2, lam=torch.full((x1.shape[0],), float(fx["lam"])), method="ddim", steps=steps, upto=upto)
    assert torch.equal(out, per), "a [B] tensor of lam and the float are one call"
    # the blend of the fixture's own latents, per element
    za, zb = (torch.as_tensor(fx[f"{o}:interp:{k}"]) for k in ("za", "zb"))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)  # noqa: E731
    mix = ops.slerp(nhwc(za), nhwc(zb), torch.full((za.shape[0],), float(fx["lam"]), device=dev)).cpu().permute(0, 3, 1, 2)
    want, mag, _, _, lerp = edit_ref.slerp(za.numpy(), zb.numpy(), [float(fx["lam"])] * za.shape[0])
    assert not lerp.any()
    assert float((np.abs(mix.double().numpy() - want) - (ROUNDINGS + 2) * U * mag).max()) <= 0.0
    parity(f"{o}: slerp of the fixture's latents against the fixture's blend", rel(mix, fx[f"{o}:interp:mix"]), 1e-6)
    # a slerp keeps the norm the latents have; the lerp of the stochastic form does not
    n = lambda t: t.flatten(1).norm(dim=1)  # noqa: E731
    assert float((n(mix) / (0.5 * (n(za) + n(zb))) - 1).abs().max()) < 0.05
    assert float((n(0.5 * (za + zb)) / (0.5 * (n(za) + n(zb)))).max()) < 0.9


# ----------------------------------------------------------------------------------------------------------------------
# graph replay against eager launches
# ----------------------------------------------------------------------------------------------------------------------
CALLS = ["encode", "decode", "img2img_ancestral", "img2img_ddim", "img2img_dpm"]


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("call", CALLS)
def test_graph_replay_equals_eager_launches(fx, nets, dev, monkeypatch, call, guided):
    from lgm_hip import sampler
    net = nets["guided"]
    img = torch.as_tensor(fx["img"]).to(dev)
    qn = torch.as_tensor(fx["q_noise"]).to(dev)
    kw = dict(classes=torch.as_tensor(fx["classes"]).to(dev), cond_scale=float(fx["cond_scale"])) if guided else {}
    if call == "img2img_ancestral":
        gd = _diffusion(net, dev, fx, "pred_v", T=int(fx["T_anc"]))
        noises = [x.to(dev) for x in torch.as_tensor(fx["anc_noises"])]
        labels, scale = gd._guidance(kw.get("classes"), kw.get("cond_scale", 1.0), img.shape[0], dev)
        run = lambda: sampler.img2img(gd, gd.normalize(img), 0.5, qn, noises=noises, classes=labels, cond_scale=scale)  # noqa: E731
    elif call.startswith("img2img"):
        gd = _diffusion(net, dev, fx, "pred_v", sampling_timesteps=10, **(dict(sampler="dpm++") if call.endswith("dpm") else {}))
        run = lambda: gd.img2img(img, 0.5, noise=qn, **kw)  # noqa: E731
    elif call == "encode":
        gd = _diffusion(net, dev, fx, "pred_v", sampling_timesteps=10)
        run = lambda: gd.encode(img, **kw)  # noqa: E731
    else:
        gd = _diffusion(net, dev, fx, "pred_v", sampling_timesteps=10)
        run = lambda: gd.decode(qn, from_level=6, clip=False, **kw)  # noqa: E731
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    before = {k for k, e in sampler._GRAPHS.get(net, {}).items() if isinstance(e, sampler._GraphedChain)}
    graph = run().clone()
    keys = {k for k, e in sampler._GRAPHS[net].items() if isinstance(e, sampler._GraphedChain)}
    assert keys, "graph capture did not happen"
    wanted = [k for k in keys if ("guided" in k) == guided and ("noclip" in k) == (call in ("encode", "decode"))
              and ("dpm++" in k) == call.endswith("dpm")]
    assert wanted, (call, guided, keys, before)
    again = run().clone()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run().clone()
    assert torch.isfinite(graph).all() and float(graph.std()) > 0
    assert torch.equal(graph, eager), f"{call}: graph replay differs from eager launches"
    assert torch.equal(graph, again), f"{call}: the second chain on one captured step differs from the first"
    if call == "encode":                                           # every frame of the eager chain: the first is the image
        frames = gd.encode(img, return_all_timesteps=True, **kw)
        assert frames.shape == (img.shape[0], 10) + tuple(img.shape[1:]) and torch.equal(frames[:, -1], graph)
        assert torch.equal(frames[:, 0], gd.normalize(img))


def test_default_interpolate_is_the_parents(fx, nets, dev):
    """``interpolate()`` without a method: the bits of the calls it has always made, written out here"""
    from lgm_hip import sampler
    gd = _diffusion(nets["plain"], dev, fx, "pred_v", T=int(fx["T_anc"]))
    x1 = torch.as_tensor(fx["img"]).to(dev) * 2 - 1
    x2 = x1.roll(1, 0)
    t, lam = 20, 0.3
    torch.manual_seed(7)
    got = gd.interpolate(x1, x2, t=t, lam=lam)
    torch.manual_seed(7)
    tb = torch.full((x1.shape[0],), t, device=dev, dtype=torch.long)
    xt1, xt2 = gd.q_sample(x1, tb), gd.q_sample(x2, tb)
    want = sampler.p_sample_loop(gd, tuple(x1.shape), init_noise=(1 - lam) * xt1 + lam * xt2, start=t, unnormalize=False)
    assert torch.equal(got, want)
    torch.manual_seed(7)
    assert torch.equal(gd.interpolate(x1, x2, t=t, lam=lam, method="stochastic"), want)


def test_module_passes_through_to_the_ema_diffusion(fx, dev):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(0)
    m = DDPM(img_channels=3, img_size=8, dim=16, sampling_timesteps=4).to(dev)
    m.prepare_hip(dev)
    img = torch.as_tensor(fx["img"]).to(dev)
    ema = m.ema.ema_model
    assert torch.equal(m.encode(img), ema.encode(img)) and torch.equal(m.reconstruct(img), ema.reconstruct(img))
    z = m.encode(img)
    assert torch.equal(m.decode(z, clip=False), ema.decode(z, clip=False))
    qn = torch.as_tensor(fx["q_noise"]).to(dev)
    assert torch.equal(m.img2img(img, strength=0.5, noise=qn), ema.img2img(img, strength=0.5, noise=qn))
