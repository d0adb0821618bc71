"""GPU: DPM-Solver++(2M) sampling (``sampler="dpm++"``; Lu et al. 2022, an extension of the reference).

  * dpm_step_kernel alone against a float64 restatement of its formula on the float32-rounded row (bounds below), its guards
    (history not read at K_1 = 0, noise not read at K_n = 0), pad lanes, in place against out of place and the table form
    against the by-value form, bit for bit;
  * whole chains against tests/golden/diffusion_dpmpp.npz (written by tools/make_golden_dpmpp.py: the solver loop around the
    REFERENCE's network and model_predictions), 1e-4 relative, a miss decided by the float64 arbiter rule of
    tests/test_hip_classcond.py; graph replay bit for bit against eager launches and against a second replay;
  * dispatch through ``GaussianDiffusion.sample``, the graph cache keys beside a DDIM step's, train.py on
    configs/diffusion/ddpm_dpmpp.json.

Measured distances go through the ``parity`` recorder (committed record: profiles/r10_dpmpp_parity.json).
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
SENTINEL = 7.0


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_dpmpp.npz")))


def _r4(n):
    return (n + 3) // 4 * 4


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    """rows of the sigmoid schedule at t = 999 (first step: K_1 = 0), 500 (every term) and 0 (the last pair: x0), SDE form,
    and the ODE row at t = 500 (K_n = 0)"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000)
    grid = [(999, 750), (750, 500), (500, 250), (250, 0), (0, -1)]
    sde, ode = sampler.dpm_coeffs(gd, grid, 2, True), sampler.dpm_coeffs(gd, grid, 2, False)
    assert sde[0][6] == 0.0 and sde[2][6] != 0.0 and sde[2][7] != 0.0 and ode[2][7] == 0.0 and ode[2][6] != 0.0
    return {999: sde[0], 500: sde[2], 0: sde[4], "ode500": ode[2]}


def _buffers(seed, B, C, HW, pitch, x_off, sc_off):
    """host buffers: x (and a self-conditioning estimate) in their slices of a sentinel-filled input buffer, the network
    output, NCHW noise, a history with sentinel pad lanes"""
    g = torch.Generator().manual_seed(seed)
    Cp = _r4(C)
    xin = torch.full((B, HW, pitch), SENTINEL)
    xin[..., x_off:x_off + C] = torch.randn(B, HW, C, generator=g) * 1.5
    if sc_off >= 0:
        xin[..., sc_off:sc_off + C] = torch.rand(B, HW, C, generator=g) * 2 - 1
    v = torch.full((B, HW, Cp), SENTINEL)
    v[..., :C] = torch.randn(B, HW, C, generator=g)
    nz = torch.randn(B, C, HW, generator=g)
    hist = torch.full((B, HW, Cp), SENTINEL)
    hist[..., :C] = torch.rand(B, HW, C, generator=g) * 2 - 1
    return xin, v, nz, hist


def _step(xin, xout, geom, v, nz, hist, objective, row, clip):
    from lgm_hip import ops
    B, C, HW, pitch, x_off, sc_off = geom
    ops.lib().lgm_dpm_step(xin.data_ptr(), xout.data_ptr(), pitch, x_off, sc_off, v.data_ptr(), v.shape[-1],
                           None if nz is None else nz.data_ptr(), hist.data_ptr(), B, C, HW, objective, row[0], row[1],
                           1 if clip else 0, *row[2:], ops.stream())
    assert ops.lib()._dll.lgm_last_kernel().decode() == "dpm_step_kernel"


def _exact(x, v, h, n, row, objective, clip):
    """float64, from the float32 row -> (next x, x0, M, m0)"""
    A, Bv, R, Rm1, Kx, K0, K1, Kn = row
    p, q = (R, Rm1) if objective == 0 else (A, -Bv)
    if objective == 1:
        x0, m0 = v.clone(), v.abs()
    else:
        x0, m0 = p * x - q * v, (p * x).abs() + (q * v).abs()
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    o = Kx * x + K0 * x0 + K1 * h + Kn * n
    return o, x0, (Kx * x).abs() + abs(K0) * m0 + (K1 * h).abs() + (Kn * n).abs(), m0


SHAPES = [(3, 3, 25, 4, 0, -1),        # 300 (pixel, lane) pairs: no multiple of 256
          (2, 3, 1024, 8, 3, 0),       # self-conditioned: slices at lanes 0 and 3 of a pitch of 8, many blocks
          (2, 1, 64, 4, 0, -1)]


@pytest.mark.parametrize("geom", SHAPES, ids=["3x3x25", "selfcond_2x3x1024", "2x1x64"])
def test_dpm_step_kernel_against_float64(dev, rows, geom):
    """Roundings on the longest path to the next x: p x, q v, their difference (x0: three, asserted against 4 u m0 with m0 =
    |p x| + |q v|, |v| for pred_x0; the clip moves nothing further away), K_0 x0, the sum with K_x x, the sum with K_1 hist,
    the sum with K_n noise - seven, each at most u relative to a partial result bounded by M = |K_x x| + |K_0| m0 + |K_1 hist|
    + |K_n noise|; asserted against 8 u M."""
    B, C, HW, pitch, x_off, sc_off = geom
    Cp = _r4(C)
    for objective in (0, 1, 2):
        for clip in (False, True):
            for t in (999, 500, 0):
                row = rows[t]
                xin, v, nz, hist = _buffers(1000 * objective + t + int(clip), B, C, HW, pitch, x_off, sc_off)
                xd, vd, nd, hd = xin.to(dev), v.to(dev), nz.to(dev), hist.to(dev)
                out = torch.full_like(xd, SENTINEL)
                _step(xd, out, geom, vd, nd, hd, objective, row, clip)
                x64 = xin[..., x_off:x_off + C].double()
                o, x0, M, m0 = _exact(x64, v[..., :C].double(), hist[..., :C].double(), nz.permute(0, 2, 1).double(), row,
                                      objective, clip)
                out, hd = out.cpu(), hd.cpu()
                what = (objective, clip, t)
                assert torch.equal(xd.cpu(), xin), "out of place: the input buffer is read only"
                assert float(((out[..., x_off:x_off + C].double() - o).abs() - 8 * U * M).max()) <= 0, what
                assert float(((hd[..., :C].double() - x0).abs() - 4 * U * m0).max()) <= 0, what
                if clip:
                    assert float(hd[..., :C].abs().max()) <= 1.0
                assert not hd[..., C:].any(), "pad lanes of the history come out zero"
                pad = torch.ones(pitch, dtype=torch.bool)
                pad[x_off:x_off + C] = False
                if sc_off >= 0:
                    pad[sc_off:sc_off + C] = False
                    assert torch.equal(out[..., sc_off:sc_off + C], hd[..., :C]), "the x0 handed to the next step"
                assert pad.any() and not out[..., pad].any(), "pad lanes of the next input buffer come out zero"
    assert Cp <= pitch


@pytest.mark.parametrize("geom", SHAPES, ids=["3x3x25", "selfcond_2x3x1024", "2x1x64"])
def test_dpm_step_kernel_guards_in_place_and_table(dev, rows, geom):
    from lgm_hip import ops
    B, C, HW, pitch, x_off, sc_off = geom
    xin, v, nz, hist = _buffers(77, B, C, HW, pitch, x_off, sc_off)
    xd, vd, nd = xin.to(dev), v.to(dev), nz.to(dev)
    nan = float("nan")
    # K_1 = 0 (the first step of a chain): a history nobody has written is not read, and holds the clipped x0 afterwards
    h_nan, out = torch.full_like(hist, nan).to(dev), torch.full_like(xd, SENTINEL)
    _step(xd, out, geom, vd, nd, h_nan, 2, rows[999], True)
    h_ok, out_ok = hist.to(dev), torch.full_like(xd, SENTINEL)
    _step(xd, out_ok, geom, vd, nd, h_ok, 2, rows[999], True)
    assert torch.isfinite(out).all() and torch.isfinite(h_nan).all()
    assert torch.equal(out, out_ok) and torch.equal(h_nan, h_ok)
    _, x0, _, m0 = _exact(xin[..., x_off:x_off + C].double(), v[..., :C].double(), torch.zeros((), dtype=torch.float64),
                          torch.zeros((), dtype=torch.float64), rows[999], 2, True)
    assert float(((h_nan.cpu()[..., :C].double() - x0).abs() - 4 * U * m0).max()) <= 0 and not h_nan[..., C:].any()
    # K_n = 0 (the ODE form, the last pair): a noise buffer is passed and not read
    n_nan = torch.full_like(nd, nan)
    for row in (rows["ode500"], rows[0]):
        a, b = torch.full_like(xd, SENTINEL), torch.full_like(xd, SENTINEL)
        ha, hb = hist.to(dev), hist.to(dev)
        _step(xd, a, geom, vd, n_nan, ha, 2, row, True)
        _step(xd, b, geom, vd, None, hb, 2, row, True)
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(ha, hb)
    # a noise pointer of NULL switches the noise term off whatever K_n is
    a, ha = torch.full_like(xd, SENTINEL), hist.to(dev)
    _step(xd, a, geom, vd, None, ha, 2, rows[500], True)
    assert torch.isfinite(a).all()
    # in place == out of place, every objective
    for objective in (0, 1, 2):
        out, ho = torch.full_like(xd, SENTINEL), hist.to(dev)
        _step(xd, out, geom, vd, nd, ho, objective, rows[500], True)
        inp, hi = xin.to(dev), hist.to(dev)
        _step(inp, inp, geom, vd, nd, hi, objective, rows[500], True)
        assert torch.equal(inp, out) and torch.equal(hi, ho), objective
    # the table form at counter 0 and at counter 2 == the by-value form with that row; advance appends counter += 1
    table = torch.zeros(4, 8)
    for i, k in enumerate((999, "ode500", 500)):
        table[i] = torch.tensor(rows[k])
    td = table.to(dev)
    for at, k in ((0, 999), (2, 500)):
        counter = torch.full((1,), at, dtype=torch.int32, device=dev)
        want, hw = xin.to(dev), hist.to(dev)
        _step(want, want, geom, vd, nd, hw, 0, rows[k], True)
        got, hg = xin.to(dev), hist.to(dev)
        ops.lib().lgm_dpm_step_table(got.data_ptr(), pitch, x_off, sc_off, vd.data_ptr(), vd.shape[-1], nd.data_ptr(),
                                     hg.data_ptr(), B, C, HW, td.data_ptr(), counter.data_ptr(), 0, 1, 1, ops.stream())
        assert ops.lib()._dll.lgm_last_kernel().decode() == "dpm_step_kernel"
        assert torch.equal(got, want) and torch.equal(hg, hw), at
        assert int(counter.item()) == at + 1


# ----------------------------------------------------------------------------------------------------------------------
# chains against the reference fixture; graph replay against eager launches
# ----------------------------------------------------------------------------------------------------------------------
KINDS = {"ode2m": dict(order=2, stochastic=False), "ode1": dict(order=1, stochastic=False),
         "sde2m": dict(order=2, stochastic=True), "selfcond": dict(order=2, stochastic=False, net="selfcond"),
         "guided": dict(order=2, stochastic=False, net="guided")}
CHAINS = [(o, k) for o in ("pred_v", "pred_noise") for k in ("ode2m", "ode1", "sde2m")] + [("pred_v", "selfcond"),
                                                                                           ("pred_v", "guided")]


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


@pytest.mark.parametrize("objective,kind", CHAINS, ids=[f"{o}-{k}" for o, k in CHAINS])
def test_chains_match_reference_fixture_and_graph_replay_equals_eager(fx, nets, dev, parity, monkeypatch, objective, kind):
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion
    from oracle import diffusion as OD
    spec = KINDS[kind]
    net = nets[spec.get("net", "plain")]
    S, B, steps = int(fx["S"]), int(fx["B"]), int(fx["steps"])
    gd = GaussianDiffusion(net, img_size=S, timesteps=int(fx["T"]), sampling_timesteps=steps, objective=objective,
                           sampler="dpm++", dpm_order=spec["order"], dpm_stochastic=spec["stochastic"]).to(dev)
    net.prepare_hip(dev)
    shape = (B, 3, S, S)
    init, nz = OD.draw_loop_noise(int(fx[f"{kind}_seed"]), shape, steps - 1)
    guided = spec.get("net") == "guided"
    y = torch.as_tensor(fx["classes"]).to(dev) if guided else None
    scale = float(fx["cond_scale"]) if guided else 1.0

    def run():
        return sampler.dpm_solver_sample(gd, shape, init_noise=init.to(dev), noises=[x.to(dev) for x in nz] + [None],
                                         classes=y, cond_scale=scale).clone()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    graph = run()
    captured = [k for k, e in sampler._GRAPHS[net].items()
                if k[:2] == ("dpm++", objective) and isinstance(e, sampler._GraphedChain) and ("guided" in k) == guided]
    assert captured, "graph capture of the DPM-Solver++ step did not happen"
    again = run()
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    eager = run()
    what = f"{objective}: 10-pair DPM-Solver++ chain, {kind}"
    assert torch.isfinite(graph).all() and float(graph.std()) > 0
    assert torch.equal(graph, eager), f"{what}: graph replay differs from eager launches"
    assert torch.equal(graph, again), f"{what}: the second chain on one captured step differs from the first"
    _arbiter(parity, f"{what}, final image", graph, fx[f"{objective}:{kind}"], fx[f"{objective}:{kind}64"])
    # the clipped x0 of the first step, as the eager chain hands it on
    chain = sampler._Chain(gd, shape, init.to(dev), None, y, scale)
    pairs = gd.dpm_time_pairs()
    row = sampler.dpm_coeffs(gd, pairs, gd.dpm_order, gd.dpm_stochastic)[0]
    sampler.dpm_step(chain, pairs[0][0], nz[0].to(dev), row)
    x0 = chain.x0[..., :3].permute(0, 3, 1, 2)
    _arbiter(parity, f"{what}, x0 of the first step", x0, fx[f"{objective}:{kind}:x0_first"],
             fx[f"{objective}:{kind}:x0_first64"])


# ----------------------------------------------------------------------------------------------------------------------
# dispatch, signatures, the graph cache beside a DDIM step
# ----------------------------------------------------------------------------------------------------------------------
def test_sample_dispatches_to_the_solver(nets, dev):
    from models.generative.diffusion.ddpm import GaussianDiffusion
    net = nets["plain"]
    gd = GaussianDiffusion(net, img_size=16, sampler="dpm++", sampling_timesteps=6).to(dev)
    net.prepare_hip(dev)
    torch.manual_seed(4)
    a = gd.sample(batch_size=2)
    assert a.shape == (2, 3, 16, 16) and torch.isfinite(a).all() and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    torch.manual_seed(4)
    frames = gd.sample(batch_size=2, return_all_timesteps=True)
    assert frames.shape == (2, 7, 3, 16, 16) and torch.isfinite(frames).all()
    assert torch.equal(frames[:, -1], a), "the last frame of the eager chain is the graph-replayed image"
    torch.manual_seed(4)
    assert torch.equal(gd.dpm_solver_sample((2, 3, 16, 16)), a)
    sde = GaussianDiffusion(net, img_size=16, sampler="dpm++", sampling_timesteps=6, dpm_stochastic=True).to(dev)
    torch.manual_seed(4)
    b = sde.sample(batch_size=2)
    assert torch.isfinite(b).all() and not torch.equal(a, b)
    # class-conditional: classes and cond_scale as the other samplers take them
    cnet = nets["guided"]
    cg = GaussianDiffusion(cnet, img_size=16, sampler="dpm++", sampling_timesteps=6, cond_scale=2.0).to(dev)
    cnet.prepare_hip(dev)
    y = torch.tensor([1, 4], device=dev)
    out = {}
    for name, kw in (("ctor", dict(classes=y)), ("two", dict(classes=y, cond_scale=2.0)), ("one", dict(classes=y, cond_scale=1.0)),
                     ("null", dict())):
        torch.manual_seed(5)
        out[name] = cg.sample(batch_size=2, **kw)
    assert torch.equal(out["ctor"], out["two"]) and not torch.equal(out["two"], out["one"])
    assert not torch.equal(out["one"], out["null"]) and all(torch.isfinite(v).all() for v in out.values())
    with pytest.raises(ValueError, match="cond_scale != 1"):
        gd.dpm_solver_sample((2, 3, 16, 16), cond_scale=2.0)


def test_ddim_graph_beside_a_dpm_graph_keeps_its_bits(fx, dev, monkeypatch):
    """a ``sampler="auto"`` diffusion on the same network, its DDIM step captured AFTER the DPM-Solver++ one: the bits of the
    eager DDIM chain (which is what its graph replay gave before this solver existed, tests/test_hip_unet.py)"""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    net = Unet(dim=16, channels=3)
    net.load_state_dict(OD.unet_init(dim=16, channels=3, seed=int(fx["seed"])), strict=True)
    auto = GaussianDiffusion(net, img_size=16, sampling_timesteps=6).to(dev)
    dpm = GaussianDiffusion(net, img_size=16, sampling_timesteps=6, sampler="dpm++").to(dev)
    net.prepare_hip(dev)
    shape = (2, 3, 16, 16)
    init = torch.randn(shape, generator=torch.Generator().manual_seed(6)).to(dev)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    before = sampler.ddim_sample(auto, shape, init_noise=init).clone()
    assert not sampler._GRAPHS.get(net)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    first = sampler.dpm_solver_sample(dpm, shape, init_noise=init).clone()
    assert [k for k in sampler._GRAPHS[net] if k[0] == "dpm++"] and len(sampler._GRAPHS[net]) == 1
    after = sampler.ddim_sample(auto, shape, init_noise=init).clone()
    keys = list(sampler._GRAPHS[net])
    assert len(keys) == 2 and all(isinstance(sampler._GRAPHS[net][k], sampler._GraphedChain) for k in keys)
    assert torch.equal(after, before), "the DDIM step captured beside the DPM-Solver++ step changed its bits"
    assert torch.equal(sampler.dpm_solver_sample(dpm, shape, init_noise=init), first) and not torch.equal(first, after)
    assert auto.sample(batch_size=2).shape == (2, 3, 16, 16)          # "auto" still dispatches to DDIM
    assert len(sampler._GRAPHS[net]) == 2


# ----------------------------------------------------------------------------------------------------------------------
# train.py
# ----------------------------------------------------------------------------------------------------------------------
def test_train_entry_runs_the_dpmpp_config(tmp_path):
    """train.py's main() on configs/diffusion/ddpm_dpmpp.json at a reduced size (16 x 16, dim 16, 20 diffusion steps, 5 solver
    steps: the step-0 sample is a 5-step chain of 64 images), three steps, in a child process with its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "ddpm_dpmpp.json")))
    assert cfg["model"]["args"]["sampler"] == "dpm++" and cfg["model"]["args"]["sampling_timesteps"] == 20
    cfg["model"]["args"].update(img_size=16, dim=16, diffusion_timesteps=20, sampling_timesteps=5)
    cfg["dataset"].update(img_size=16, batch_size=8)
    path = tmp_path / "ddpm_dpmpp_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_ddpm_dpmpp"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('LAST_SAMPLES', tuple(m.last_samples.shape), bool(torch.isfinite(m.last_samples).all())); "
            "print('SAMPLER', m.ema.ema_model.sampler, m.ema.ema_model.sampling_timesteps); "
            "print('TRAIN_LOSS', float(m.logged['train_loss']))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--max_steps", "3", "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("LAST_SAMPLES", "TRAIN_LOSS", "SAMPLER"))}
    assert lines["LAST_SAMPLES"] == "LAST_SAMPLES (64, 3, 16, 16) True", lines
    assert lines["SAMPLER"] == "SAMPLER dpm++ 5"
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 3 and sd["hyper_parameters"]["sampler"] == "dpm++"
