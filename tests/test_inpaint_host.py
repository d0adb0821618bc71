"""CPU: the host side of inpainting (RePaint, Lugmayr et al. 2022, Algorithm 1; ``GaussianDiffusion.inpaint``).

  * ``inpaint_walk`` against five walks written out by hand, its ValueErrors, the folding of a jump into the step before it;
  * ``_plan_inpaint``: resamples = 1 is the sampler's own plan with (M_a, M_n, 1, 0) beside it, the jump weights against the
    float64 product of 1 - beta, J_x^2 + J_n^2 = 1, DPM-Solver++ first-order after every jump;
  * ``_segments`` over the 9,910 steps of (1000, 10, 10), the graph key, the eager launch trace under a recorder;
  * the new entry points: declared, exported, behind the two existing kernels, argument checks;
  * ``GaussianDiffusion.inpaint``'s own argument checks.
"""
import ctypes
import math
import subprocess

import pytest
import torch

U = 2.0 ** -24                        # unit roundoff of float32
WALKS = {(4, 2, 2): [3, 2, 1, 0, 1, 2, 1, 0, -1],
         (6, 2, 2): [5, 4, 3, 2, 3, 4, 3, 2, 1, 0, 1, 2, 1, 0, -1],
         (5, 1, 2): [4, 3, 4, 3, 2, 3, 2, 1, 2, 1, 0, 1, 0, -1],
         (4, 2, 1): [3, 2, 1, 0, -1]}
FORWARDS = {(4, 2, 2): 6, (6, 2, 2): 10, (5, 1, 2): 9, (4, 2, 1): 4, (1000, 10, 10): 9910}
ENTRIES = {"lgm_sample_step_inpaint": 36, "lgm_dpm_step_inpaint": 35}


def _f32(x):
    return float(torch.as_tensor(x, dtype=torch.float32))


def _gd(kind, **kw):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    args = {"ancestral": dict(timesteps=20),
            "ddim0": dict(timesteps=1000, sampling_timesteps=10),
            "ddim1": dict(timesteps=1000, sampling_timesteps=10, ddim_sampling_eta=1.0),
            "dpm": dict(timesteps=1000, sampling_timesteps=10, sampler="dpm++"),
            "dpm_sde": dict(timesteps=1000, sampling_timesteps=10, sampler="dpm++", dpm_stochastic=True)}[kind]
    return GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, **dict(args, **kw))


def test_the_five_walks():
    from lgm_hip import sampler
    for args, want in WALKS.items():
        assert sampler.inpaint_walk(*args) == want, args
    big = sampler.inpaint_walk(1000, 10, 10)
    assert len(big) == 18821 and big[0] == 999 and big[-2:] == [0, -1] and max(big) == 999 and min(big[:-1]) == 0
    for args, n in FORWARDS.items():
        levels = sampler.inpaint_walk(*args)
        steps = sampler.inpaint_steps(levels)
        assert len(steps) == n, args
        # one step per move down; a jump is folded into the step before it and never stands alone
        assert sum(1 for a, b in zip(levels, levels[1:]) if b == a - 1) == n
        flat = []
        for l, s, u in steps:
            assert s == l - 1 and u >= s and (u == s or (u - s == args[1] and s >= 0))
            flat += [l] + list(range(s, u))
        assert flat + [-1] == levels


def test_walk_value_errors():
    from lgm_hip import sampler
    for args in ((4, 0, 2), (4, -1, 1), (4, 2, 0), (4, 5, 2), (0, 1, 1)):
        with pytest.raises(ValueError):
            sampler.inpaint_walk(*args)
    assert sampler.inpaint_walk(4, 5, 1) == [3, 2, 1, 0, -1]         # jump_length > n without resampling: nothing jumps
    assert sampler.inpaint_walk(4, 4, 3) == [3, 2, 1, 0, -1]         # range(0, 0): no level jumps
    with pytest.raises(ValueError):
        sampler.inpaint_steps([2, 3, 2, 1, 0, -1])                   # an up move that stands alone


@pytest.mark.parametrize("kind", ["ancestral", "ddim0", "ddim1", "dpm", "dpm_sde"])
def test_one_resample_is_the_plain_plan_with_the_known_weights_beside_it(kind):
    from lgm_hip import sampler
    gd = _gd(kind)
    base = {"ancestral": sampler._plan_ancestral, "ddim0": sampler._plan_ddim, "ddim1": sampler._plan_ddim,
            "dpm": sampler._plan_dpm, "dpm_sde": sampler._plan_dpm}[kind](gd)
    for jump in (1, 3):
        plan = sampler._plan_inpaint(gd, jump, 1)
        assert (plan.times, plan.rows, plan.draws, plan.with_noise, plan.rederive, plan.dpm) == \
               (base.times, base.rows, base.draws, base.with_noise, base.rederive, base.dpm)
        assert base.irows is None and len(plan.irows) == len(plan.rows)
        acp = gd.alphas_cumprod.double()
        nexts = list(plan.times[1:]) + [-1]
        for row, s in zip(plan.irows, nexts):
            want = (1.0, 0.0) if s < 0 else (_f32(acp[s].sqrt()), _f32((1 - acp[s]).sqrt()))
            assert row == want + (1.0, 0.0)
        assert plan.kdraws == tuple(s >= 0 for s in nexts) and plan.jdraws == (False,) * len(nexts)


def test_jump_weights_of_the_ancestral_grid():
    """J_x^2 = acp[u] / acp[s] is the product of 1 - beta over the jumped levels.  Tolerance: alphas_cumprod and betas are
    float32 tables (one rounding u each: 2 u on the ratio, j u on a product of j factors 1 - beta, j = 5 here), J_x is
    rounded once (2 u on its square): 9 u in all, taken as 12 u; J_x^2 + J_n^2 = 1 within 2 u (J_x^2) + 2 u (J_n^2)."""
    from lgm_hip import sampler
    gd = _gd("ancestral")
    plan = sampler._plan_inpaint(gd, 5, 2)
    steps = sampler.inpaint_steps(sampler.inpaint_walk(20, 5, 2))
    assert len(steps) == len(plan.irows) == 35 and plan.times == tuple(l for l, _, _ in steps)
    one_minus_beta = (1.0 - gd.betas.double()).tolist()
    jumps = 0
    for (l, s, u), (ma, mn, jx, jn), row in zip(steps, plan.irows, plan.rows):
        assert row == sampler._p_sample_coeffs(gd, l)
        if u == s:
            assert (jx, jn) == (1.0, 0.0)
            continue
        jumps += 1
        prod = math.prod(one_minus_beta[s + 1:u + 1])
        assert u - s == 5 and abs(jx * jx - prod) <= 12 * U * prod, (s, u, jx * jx, prod)
        assert abs(jx * jx + jn * jn - 1.0) <= 4 * U
        assert abs(ma * ma + mn * mn - 1.0) <= 4 * U
    assert jumps == 3
    assert plan.jdraws == tuple(u != s for _, s, u in steps) and plan.kdraws == tuple(s >= 0 for _, s, _ in steps)
    assert plan.draws == tuple(l > 0 for l, _, _ in steps) and plan.with_noise


@pytest.mark.parametrize("kind", ["ddim0", "ddim1", "dpm", "dpm_sde"])
def test_plans_on_the_ddim_grid(kind):
    from lgm_hip import sampler
    gd = _gd(kind)
    pairs = gd.ddim_time_pairs()
    grid = sampler.inpaint_grid(gd, "dpm" if kind.startswith("dpm") else "ddim")
    assert grid == [t for t, _ in reversed(pairs)] and len(grid) == 10
    plan = sampler._plan_inpaint(gd, 3, 2)
    steps = sampler.inpaint_steps(sampler.inpaint_walk(10, 3, 2))
    assert len(plan.rows) == len(plan.irows) == len(steps) == 19
    time = lambda l: grid[l] if l >= 0 else -1  # noqa: E731
    acp = gd.alphas_cumprod.double()
    after_jump = False
    for i, ((l, s, u), row, irow) in enumerate(zip(steps, plan.rows, plan.irows)):
        assert plan.times[i] == time(l) and len(row) == 8 and len(irow) == 4
        assert row[:4] == sampler._head(sampler._host_schedule(gd), time(l))
        if kind.startswith("ddim"):
            assert row == sampler._ddim_coeffs(gd, time(l), time(s), gd.ddim_sampling_eta)
        else:
            # every monotone run is a solver chain of its own: first-order (K_1 == 0) at the start and after every jump,
            # second-order inside a run
            first = i == 0 or after_jump
            assert (row[6] == 0.0) == (first or s < 0), (i, row)
            if first and s >= 0:
                assert row == sampler.dpm_coeffs(gd, [(time(l), time(s))], 2, gd.dpm_stochastic)[0]
        after_jump = u != s
        if u != s:
            ratio = float(acp[time(u)] / acp[time(s)])
            assert irow[2:] == (_f32(math.sqrt(ratio)), _f32(math.sqrt(1 - ratio)))
            assert abs(irow[2] ** 2 + irow[3] ** 2 - 1.0) <= 4 * U
        else:
            assert irow[2:] == (1.0, 0.0)
    assert sum(plan.jdraws) == 3 and plan.rederive == kind.startswith("ddim") and plan.dpm == kind.startswith("dpm")
    assert plan.with_noise == (kind in ("ddim1", "dpm_sde"))


def test_segments_cover_a_long_walk_once():
    from lgm_hip import sampler
    n = len(sampler.inpaint_steps(sampler.inpaint_walk(1000, 10, 10)))
    assert n == 9910
    for max_steps in (4096, 1, 9910, 9909, 7):
        segs = sampler._segments(n, max_steps)
        assert [i for lo, hi in segs for i in range(lo, hi)] == list(range(n))
        assert all(0 < hi - lo <= max_steps for lo, hi in segs)
    assert sampler._segments(n, 4096) == [(0, 4096), (4096, 8192), (8192, 9910)]
    assert sampler._segments(10, 4096) == [(0, 10)] and sampler._segments(0, 4096) == []
    with pytest.raises(ValueError):
        sampler._segments(5, 0)


def test_graph_key_gets_an_inpaint_component():
    from lgm_hip import sampler
    S = (2, 3, 16, 16)
    gd = _gd("dpm")
    plain = sampler._graph_key(gd, S, False, False, False, True)
    assert plain == ("dpm++", "pred_v", S, False) == sampler._graph_key(gd, S, False, False, False, True, False)
    assert sampler._graph_key(gd, S, False, False, False, True, True) == ("inpaint",) + plain
    thr = _gd("ancestral", dynamic_thresholding=True)
    assert sampler._graph_key(thr, S, True, False, True, False, True) == ("inpaint", "dynthresh", 0.995, S, True, "guided")


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lgm_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.mark.parametrize("kind,self_condition,dyn", [("ancestral", False, False), ("ddim1", True, False), ("dpm", False, True),
                                                      ("dpm_sde", True, False)])
def test_eager_launch_trace(monkeypatch, kind, self_condition, dyn):
    """the eager chain under a recorder: per step one forward and ONE update launch (one more when thresholded), the rows by
    value, the draws in the order noise, eps_k, eps_j and handed in only where their weight is not zero"""
    from lgm_hip import ops, sampler
    from models.generative.diffusion.ddpm import OBJECTIVES, GaussianDiffusion, Unet
    shape = B, C, H, W = (2, 3, 4, 4)
    args = {"ancestral": dict(timesteps=6), "ddim1": dict(timesteps=6, sampling_timesteps=4, ddim_sampling_eta=1.0),
            "dpm": dict(timesteps=6, sampling_timesteps=4, sampler="dpm++"),
            "dpm_sde": dict(timesteps=6, sampling_timesteps=4, sampler="dpm++", dpm_stochastic=True)}[kind]
    gd = GaussianDiffusion(Unet(dim=16, channels=C, self_condition=self_condition), img_size=H, dynamic_thresholding=dyn, **args)
    net, rec, vs, drawn, chains = gd.model, _Recorder(), [], [], []
    monkeypatch.setattr(ops, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream", lambda: 0)
    monkeypatch.setattr(net, "prepare_hip", lambda device: None)

    def forward(x, t, classes=None, cond_scale=1.0, **kw):
        vs.append((torch.zeros(x.shape[:3] + (4,)), x, t.tolist()))
        return vs[-1][0]
    monkeypatch.setattr(net, "forward_guided", forward)
    randn, chain_cls = torch.randn, sampler._Chain

    def counting_randn(*a, **kw):
        drawn.append(randn(*a, **kw))
        return drawn[-1]

    def chain(*a, **kw):
        chains.append(chain_cls(*a, **kw))
        return chains[-1]
    monkeypatch.setattr(sampler.torch, "randn", counting_randn)
    monkeypatch.setattr(sampler, "_Chain", chain)
    known, mask = torch.zeros(shape), torch.ones(B, 1, H, W)
    plan = sampler._plan_inpaint(gd, 2, 2)
    n = len(plan.times)
    assert n == len(sampler.inpaint_steps(sampler.inpaint_walk(6 if kind == "ancestral" else 4, 2, 2)))
    out = sampler.inpaint(gd, known, mask, 2, 2)
    (ch,) = chains
    assert tuple(out.shape) == shape and tuple(ch.known.shape) == (B, H, W, 4) and tuple(ch.mask.shape) == (B, H * W)
    flags = list(zip(plan.draws, plan.kdraws, plan.jdraws))
    assert len(drawn) == 1 + sum(sum(f) for f in flags)
    it = iter(drawn[1:])
    updates = [(name, a) for name, a in rec.calls if name.endswith("_inpaint")]
    others = [name for name, _ in rec.calls if not name.endswith("_inpaint")]
    assert others.count("lgm_dyn_thresh") == (n if dyn else 0) and len(updates) == n == len(vs)
    assert set(others) <= {"lgm_nchw_to_nhwc", "lgm_nhwc_to_nchw", "lgm_dyn_thresh"}
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    dpm = kind.startswith("dpm")
    for i, ((name, a), (v, x, ts), row, irow, f) in enumerate(zip(updates, vs, plan.rows, plan.irows, flags)):
        nz, ek, ej = (next(it) if g else None for g in f)
        assert name == ("lgm_dpm_step_inpaint" if dpm else "lgm_sample_step_inpaint") and ts == [plan.times[i]] * B
        assert len(a) == ENTRIES[name] and a[0] == x.data_ptr() and a[1] != a[0]
        assert a[2:8] == (net.in_pitch, net.x_off, net.sc_off, v.data_ptr(), 4, ptr(nz if row[7] != 0.0 else None))
        tail = a[-14:]
        assert tail == (None, None, 0, ptr(ch.thresh), ptr(ch.known), ptr(ch.mask), ptr(ek), ptr(ej), *irow, None, 0)
        head = a[8:-14]
        if dpm:
            assert head == (ptr(ch.hist), B, C, H * W, OBJECTIVES["pred_v"], *row)
        else:
            x0 = None if self_condition else ptr(chains[0].x0 if not self_condition else None)
            assert head == (x0, B, C, H * W, OBJECTIVES["pred_v"], 1 if kind.startswith("ddim") else 0, *row)


def test_entry_points_are_declared_exported_and_check_their_arguments():
    from lgm_hip import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert name in protos, f"{name} is not declared in include/lgm_hip.h"
        assert hasattr(dll, name), f"{name} is not exported by the library"
        assert len(protos[name][1]) == nargs, name
        assert protos[name][0] is ctypes.c_int and protos[name][1][-1] is ctypes.c_void_p
    fl, vp, i32 = ctypes.c_float, ctypes.c_void_p, ctypes.c_int
    assert protos["lgm_sample_step_inpaint"][1][-14:] == [vp, vp, i32, vp, vp, vp, vp, vp, fl, fl, fl, fl, vp, vp]
    assert protos["lgm_dpm_step_inpaint"][1][-14:] == [vp, vp, i32, vp, vp, vp, vp, vp, fl, fl, fl, fl, vp, vp]
    L = _lib.lib()
    assert L.lgm_abi_version() == _lib.ABI_VERSION == 8
    syms = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for kernel in ("sample_step_slice_kernel(", "dpm_step_kernel("):     # the two kernels there were, and no third
        assert kernel in syms
    assert "inpaint_kernel" not in syms and "inpaint_step_kernel" not in syms
    # the host rejects bad arguments before any launch (no GPU needed)
    buf = (ctypes.c_float * 512)()
    p = ctypes.addressof(buf)
    q, h, v, th, kn, mk, ek, ej, tb = (p + 64 * k for k in range(1, 10))
    row, irow = (0.5, -0.5, 2.0, 1.0, 0.5, 0.5, 0.0, 0.0), (0.5, 0.5, 0.9, 0.1)

    def step(xin=p, xout=q, sc_off=-1, v=v, objective=2, table=None, counter=None, advance=0, known=kn, mask=mk, eps_k=ek,
             eps_j=ej, irow=irow, itable=None, x_off=0):
        L.lgm_sample_step_inpaint(xin, xout, 4, x_off, sc_off, v, 4, None, None, 1, 3, 1, objective, 0, *row, table, counter,
                                  advance, None, known, mask, eps_k, eps_j, *irow, itable, None)

    def dpm(xin=p, xout=q, hist=h, v=v, objective=2, table=None, counter=None, advance=0, known=kn, mask=mk, eps_k=ek,
            eps_j=ej, irow=irow, itable=None):
        L.lgm_dpm_step_inpaint(xin, xout, 4, 0, -1, v, 4, None, hist, 1, 3, 1, objective, *row, table, counter, advance, None,
                               known, mask, eps_k, eps_j, *irow, itable, None)
    bad = (dict(xin=None), dict(v=None), dict(objective=3), dict(known=None), dict(mask=None),      # a mask without known ...
           dict(known=None, mask=None), dict(eps_k=None), dict(eps_j=None),                          # ... draws without it
           dict(table=tb, counter=tb), dict(itable=tb), dict(table=tb, counter=tb, itable=tb),      # tables: both, in place
           dict(xout=p, table=tb, counter=tb, itable=tb, eps_k=None), dict(advance=1), dict(known=p), dict(mask=q))
    for kw in bad:
        with pytest.raises(_lib.LgmArgumentError, match="sample_step_inpaint"):
            step(**kw)
        with pytest.raises(_lib.LgmArgumentError, match="dpm_step_inpaint"):
            dpm(**kw)
    for kw in (dict(x_off=2), dict(sc_off=2)):
        with pytest.raises(_lib.LgmArgumentError, match="sample_step_inpaint"):
            step(**kw)
    with pytest.raises(_lib.LgmArgumentError, match="dpm_step_inpaint"):
        dpm(hist=p)
    with pytest.raises(_lib.LgmArgumentError, match="dpm_step_inpaint"):
        dpm(known=h)


def test_public_inpaint_checks_its_arguments():
    from models.generative.diffusion.ddpm import DDPM, GaussianDiffusion
    gd = _gd("ddim0")
    known = torch.rand(2, 3, 16, 16)
    for mask in (torch.ones(2, 16, 16) * 1.5, -torch.ones(2, 1, 16, 16), torch.full((2, 1, 16, 16), float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            gd.inpaint(known, mask)
    for mask in (torch.ones(2, 3, 16, 16), torch.ones(1, 1, 16, 16), torch.ones(2, 16, 8), torch.ones(2, 256)):
        with pytest.raises(ValueError, match="mask must be"):
            gd.inpaint(known, mask)
    for bad in (torch.rand(2, 1, 16, 16), torch.rand(2, 3, 8, 16), torch.rand(3, 16, 16)):
        with pytest.raises(ValueError, match="known must be"):
            gd.inpaint(bad, torch.ones(2, 1, 16, 16))
    with pytest.raises(ValueError):
        gd.inpaint(known, torch.ones(2, 1, 16, 16), jump_length=0)
    with pytest.raises(ValueError):
        gd.inpaint(known, torch.ones(2, 1, 16, 16), jump_length=11, resamples=2)
    assert callable(DDPM.inpaint) and callable(GaussianDiffusion.inpaint)
