"""CPU: the launch trace of the eager sampling chains.  The library is replaced by a recorder (the pattern of
tests/test_cpu_objectives.py), the network forward by zeros; without a device ``_graph_chain`` answers None, so the public
loops of ``lgm_hip.sampler`` run their eager path end to end.  Every case pins the ordered entry points of the whole chain,
every scalar argument, every pointer argument by its role in the chain (x / x_next / x0 / hist / thresh / the step's noise)
and the number of ``torch.randn`` calls.  Table mode of the shared update launch and the graph cache keys are pinned at the
end of the file."""
import ctypes

import pytest
import torch

SHAPE = (2, 3, 4, 4)
B, C, H, W = SHAPE
HW, CP, T = H * W, 4, 6
SAMPLERS = {"ancestral": dict(),
            "ddim_eta0": dict(sampling_timesteps=3, ddim_sampling_eta=0.0),
            "ddim_eta1": dict(sampling_timesteps=3, ddim_sampling_eta=1.0),
            "dpm_ode": dict(sampling_timesteps=3, sampler="dpm++"),
            "dpm_sde": dict(sampling_timesteps=3, sampler="dpm++", dpm_stochastic=True)}


class _Recorder:
    """Stands in for the library: records (entry point, arguments) of every call and answers 0 (launched).  The one thing it
    computes: ``lgm_nhwc_to_nchw`` zero-fills its destination, so that an image is 0 and an unnormalised one 0.5."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lgm_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == "lgm_nhwc_to_nchw":
                ctypes.memset(args[2], 0, 4 * args[3] * args[4] * args[5])
            return 0
        return call


class _Session:
    """One sampling run under the recorder: the chain the loop built, the buffers it started with, the network outputs and
    the tensors ``torch.randn`` returned, in order."""

    def __init__(self, monkeypatch):
        from lgm_hip import ops, sampler
        self.sampler, self.mp = sampler, monkeypatch
        self.rec = _Recorder()
        self.chains, self.bufs, self.vs, self.fwd, self.drawn = [], [], [], [], []
        monkeypatch.setattr(ops, "lib", lambda: self.rec)
        monkeypatch.setattr(ops, "stream", lambda: 0)
        randn, chain_cls = torch.randn, sampler._Chain

        def counting_randn(*a, **kw):
            self.drawn.append(randn(*a, **kw))
            return self.drawn[-1]

        def chain(*a, **kw):
            ch = chain_cls(*a, **kw)
            self.chains.append(ch)
            self.bufs.append((ch.x, ch.x_next, ch.x0, ch.thresh))
            return ch
        monkeypatch.setattr(sampler.torch, "randn", counting_randn)      # the name the module draws through
        monkeypatch.setattr(sampler, "_Chain", chain)

    def diffusion(self, kind, objective, self_condition, dyn):
        from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
        gd = GaussianDiffusion(Unet(dim=16, channels=C, self_condition=self_condition), img_size=H, timesteps=T,
                               objective=objective, dynamic_thresholding=dyn, **SAMPLERS[kind])
        net = gd.model

        def forward(x, t, classes=None, cond_scale=1.0, **kw):
            self.fwd.append((x, t.tolist(), classes, cond_scale, kw))
            self.vs.append(torch.zeros(x.shape[:3] + (CP,)))
            return self.vs[-1]
        self.mp.setattr(net, "prepare_hip", lambda device: None)
        self.mp.setattr(net, "forward_guided", forward)
        self.drawn.clear()                       # building the network drew its parameters; the count is the sampler's
        return gd


@pytest.fixture
def session(monkeypatch):
    return _Session(monkeypatch)


def _f32(x):
    return float(torch.as_tensor(x, dtype=torch.float32))


def _plan(sampler, kind, gd, start=None):
    """-> [(t, row of 8, draws)], rederive, dpm: the steps of a chain, the conditions restated from the loops"""
    if kind == "ancestral":
        ts = list(reversed(range(T if start is None else start)))
        return [(t, sampler._p_sample_coeffs(gd, t), t > 0) for t in ts], 0, False
    pairs = gd.ddim_time_pairs()
    assert pairs == [(5, 3), (3, 1), (1, -1)]
    if kind.startswith("ddim"):
        eta = gd.ddim_sampling_eta
        return [(t, sampler._ddim_coeffs(gd, t, s, eta), s >= 0 and eta != 0.0) for t, s in pairs], 1, False
    rows = sampler.dpm_coeffs(gd, pairs, gd.dpm_order, gd.dpm_stochastic)
    return [(t, row, s >= 0 and gd.dpm_stochastic) for (t, s), row in zip(pairs, rows)], 0, True


def _run_and_check(ses, kind, objective, self_condition, dyn, frames=False, start=None, unnormalize=None, given=False):
    """Run the public loop of ``kind`` and compare the whole trace with the one written out here."""
    from models.generative.diffusion.ddpm import OBJECTIVES
    sampler = ses.sampler
    gd = ses.diffusion(kind, objective, self_condition, dyn)
    net, obj = gd.model, OBJECTIVES[objective]
    pitch, x_off, sc_off = (net.in_pitch, net.x_off, net.sc_off)
    assert (pitch, x_off, sc_off) == ((8, 3, 0) if self_condition else (4, 0, -1))
    steps, rederive, dpm = _plan(sampler, kind, gd, start)
    n = len(steps)
    hs = {k: getattr(gd, k) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                                      "sqrt_recipm1_alphas_cumprod")}
    for t, row, _ in steps:                      # the head of every row, spelled independently of the module
        assert len(row) == 8 and all(isinstance(c, float) for c in row)
        assert tuple(row[:4]) == (_f32(hs["sqrt_alphas_cumprod"][t]), -_f32(hs["sqrt_one_minus_alphas_cumprod"][t]),
                                  _f32(hs["sqrt_recip_alphas_cumprod"][t]), _f32(hs["sqrt_recipm1_alphas_cumprod"][t]))
    kw = {}
    if given:                                    # the caller's tensors: no draw at all
        kw = dict(init_noise=torch.zeros(SHAPE), noises=[torch.zeros(SHAPE) for _ in range(n)])
    if start is not None:
        kw.update(start=start, unnormalize=unnormalize)
    loop = sampler.dpm_solver_sample if dpm else sampler.p_sample_loop if kind == "ancestral" else sampler.ddim_sample
    out = loop(gd, SHAPE, frames, **kw)

    (ch,), ((X0, X1, x0buf, thresh),) = ses.chains, ses.bufs
    init = kw["init_noise"] if given else ses.drawn[0]
    drawn = iter(kw["noises"] if given else ses.drawn[1:])
    noise_of = []
    for i, (t, row, draws) in enumerate(steps):
        nz = None
        if draws:
            nz = kw["noises"][i] if given else next(drawn)
        noise_of.append(nz if (kind == "ancestral" or row[7] != 0.0) else None)
    # the number and order of the draws: the start image, then one per drawing step
    assert len(ses.drawn) == (0 if given else 1 + sum(1 for _, _, d in steps if d))
    assert all(tuple(d.shape) == SHAPE for d in ses.drawn)
    if kind in ("ancestral", "ddim_eta1", "dpm_sde"):
        assert sum(1 for nz in noise_of if nz is not None) == max(n - 1, 0) and (not n or noise_of[-1] is None)
    else:
        assert noise_of == [None] * n

    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    assert (thresh is not None) == dyn and (x0buf is None) == self_condition
    assert (ch.hist is not None) == dpm and (not dpm or tuple(ch.hist.shape) == (B, H, W, CP))
    k_w = sampler.dyn_rank(C * HW, gd.dynamic_thresholding_percentile) if dyn else None
    image = lambda x: ("lgm_nhwc_to_nchw", (net.x_slice(x).data_ptr(), pitch, None, B, C, HW, 0))  # noqa: E731
    want = [("lgm_nchw_to_nhwc", (ptr(init), net.x_slice(X0, pad=True).data_ptr() if self_condition else ptr(X0), pitch,
                                  B, C, HW, pitch - x_off, 0))]
    if frames:
        want.append(image(X0))
    for i, ((t, row, _), nz) in enumerate(zip(steps, noise_of)):
        x, xn = (X0, X1) if i % 2 == 0 else (X1, X0)
        v = ses.vs[i]
        fx, ft, fcls, fscale, fkw = ses.fwd[i]
        assert fx is x and ft == [t] * B and fcls is None and fscale == 1.0 and not fkw
        head, tail = tuple(row[:4]), tuple(row[4:])
        pre = (ptr(x), ptr(xn), pitch, x_off, sc_off, ptr(v), CP, ptr(nz))
        if dyn:
            want.append(("lgm_dyn_thresh", (ptr(x), pitch, x_off, ptr(v), CP, B, C, HW, obj, *head, None, None, *k_w,
                                            ptr(thresh), 0)))
        if dpm and dyn:
            want.append(("lgm_dpm_step_thresh", pre + (ptr(ch.hist), B, C, HW, obj, *head, *tail, None, None, 0, ptr(thresh), 0)))
        elif dpm:
            want.append(("lgm_dpm_step", pre + (ptr(ch.hist), B, C, HW, obj, head[0], head[1], 1, head[2], head[3], *tail, 0)))
        elif dyn:
            want.append(("lgm_sample_step_thresh", pre + (None if self_condition else ptr(x0buf), B, C, HW, obj, rederive,
                                                          *head, *tail, None, None, 0, ptr(thresh), 0)))
        elif self_condition:
            want.append(("lgm_sample_step_slice", pre + (B, C, HW, obj, head[0], head[1], 1, rederive, head[2], head[3],
                                                         *tail, 0)))
        else:
            want.append(("lgm_sample_step_obj", (ptr(x), ptr(v), ptr(nz), ptr(xn), ptr(x0buf), B, C, HW, CP, obj, head[0],
                                                 head[1], 1, rederive, head[2], head[3], *tail, 0)))
        if frames:
            want.append(image(xn))
    last = X0 if n % 2 == 0 else X1
    if not frames:
        want.append(image(last))
    got = ses.rec.calls
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, args), (_, wargs) in zip(got, want):
        if name == "lgm_nhwc_to_nchw":           # the destination is a tensor of the call's own
            args = args[:2] + (None,) + args[3:]
        assert args == wargs, name
    assert len(ses.vs) == n

    # the state a step leaves behind
    assert ch.x is last and ch.x_next is (X1 if last is X0 else X0)
    if n and self_condition:
        assert ch.x0.data_ptr() == net.sc_slice(last).data_ptr()
    elif n:
        assert ch.x0 is (ch.hist if dpm else x0buf)
    # the result: zeros from the recorder's nhwc_to_nchw, unnormalised to 0.5 once
    unn = gd.auto_normalize if unnormalize is None else unnormalize
    assert tuple(out.shape) == ((B, n + 1, C, H, W) if frames else SHAPE)
    assert torch.equal(out, torch.full_like(out, 0.5 if unn else 0.0))
    if not frames:
        assert got[-1][1][2] == out.data_ptr()
    return ch


@pytest.mark.parametrize("dyn", [False, True], ids=["clamp", "dynthresh"])
@pytest.mark.parametrize("self_condition", [False, True], ids=["plain", "selfcond"])
@pytest.mark.parametrize("objective", ["pred_noise", "pred_v"])
@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_eager_chain_trace(session, kind, objective, self_condition, dyn):
    _run_and_check(session, kind, objective, self_condition, dyn)


@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_eager_chain_trace_with_every_frame(session, kind):
    _run_and_check(session, kind, "pred_noise", True, True, frames=True)


@pytest.mark.parametrize("kind", ["ancestral", "ddim_eta1", "dpm_sde"])
def test_eager_chain_trace_with_the_callers_noise(session, kind):
    _run_and_check(session, kind, "pred_v", False, False, given=True)


@pytest.mark.parametrize("given", [False, True])
def test_ancestral_chain_from_a_start_step_without_unnormalising(session, given):
    """what ``interpolate`` asks for: steps start - 1 .. 0 and the image left in [-1, 1]"""
    _run_and_check(session, "ancestral", "pred_v", True, False, start=4, unnormalize=False, given=given)


def test_an_empty_ancestral_chain_launches_no_step(session):
    _run_and_check(session, "ancestral", "pred_noise", False, False, start=0, unnormalize=True)


@pytest.mark.parametrize("noisy", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("self_condition", [False, True], ids=["plain", "selfcond"])
@pytest.mark.parametrize("dyn", [False, True], ids=["clamp", "dynthresh"])
@pytest.mark.parametrize("dpm", [False, True], ids=["step", "dpm"])
def test_update_launch_in_table_mode(session, dpm, dyn, self_condition, noisy):
    """the captured step's call of the shared update launch: the row read from table[counter], zeros in the by-value slots,
    clip = 1 and advance = 1, in place in the static buffer, no x0 output; the threshold launch reads the same table row"""
    from models.generative.diffusion.ddpm import OBJECTIVES
    sampler = session.sampler
    gd = session.diffusion("dpm_sde" if dpm else "ddim_eta1", "pred_noise", self_condition, dyn)
    net, obj = gd.model, OBJECTIVES["pred_noise"]
    x, v = torch.zeros(B, H, W, net.in_pitch), torch.zeros(B, H, W, CP)
    table, counter = torch.zeros(16, 8), torch.zeros(1, dtype=torch.int32)
    hist, thresh, nz = torch.zeros(B, H, W, CP), torch.zeros(B), torch.zeros(SHAPE) if noisy else None
    rank = sampler.dyn_rank(C * HW, 0.995) if dyn else None
    for rederive in ((False,) if dpm else (False, True)):
        session.rec.calls.clear()
        sampler._launch_update(net, SHAPE, obj, v, nz, x=x, x_next=x, hist=hist if dpm else None,
                               thresh=thresh if dyn else None, rank=rank, table=table, counter=counter, rederive=rederive,
                               dpm=dpm)
        src = (net.in_pitch, net.x_off, net.sc_off, v.data_ptr(), CP, None if nz is None else nz.data_ptr())
        tab, zeros = (table.data_ptr(), counter.data_ptr()), (0.0,) * 8
        if dyn:
            want = [("lgm_dyn_thresh", (x.data_ptr(), net.in_pitch, net.x_off, v.data_ptr(), CP, B, C, HW, obj, 0.0, 0.0, 0.0,
                                        0.0, *tab, *rank, thresh.data_ptr(), 0))]
            if dpm:
                want.append(("lgm_dpm_step_thresh", (x.data_ptr(), x.data_ptr(), *src, hist.data_ptr(), B, C, HW, obj, *zeros,
                                                     *tab, 1, thresh.data_ptr(), 0)))
            else:
                want.append(("lgm_sample_step_thresh", (x.data_ptr(), x.data_ptr(), *src, None, B, C, HW, obj, int(rederive),
                                                        *zeros, *tab, 1, thresh.data_ptr(), 0)))
        elif dpm:
            want = [("lgm_dpm_step_table", (x.data_ptr(), *src, hist.data_ptr(), B, C, HW, *tab, obj, 1, 1, 0))]
        else:
            want = [("lgm_sample_step_table_slice", (x.data_ptr(), *src, B, C, HW, *tab, obj, 1, int(rederive), 1, 0))]
        assert session.rec.calls == want


def test_graph_keys():
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    S = (2, 3, 4, 4)
    net = Unet(dim=16, channels=3)
    mk = lambda objective, **kw: GaussianDiffusion(net, img_size=4, timesteps=6, objective=objective, **kw)  # noqa: E731
    v, eps = mk("pred_v"), mk("pred_noise")
    assert sampler._graph_key(v, S, True, False, False, False) == (S, True)                       # ancestral
    assert sampler._graph_key(v, list(S), False, True, False, False) == (S, False)                # DDIM, eta 0
    assert sampler._graph_key(eps, S, False, True, False, False) == (S, False, "pred_noise", True)
    assert sampler._graph_key(eps, S, False, True, True, False) == (S, False, "pred_noise", True, "guided")
    assert sampler._graph_key(eps, S, False, False, False, True) == ("dpm++", "pred_noise", S, False, "pred_noise", False)
    thr = mk("pred_v", sampling_timesteps=3, sampler="dpm++", dpm_stochastic=True, dynamic_thresholding=True,
             dynamic_thresholding_percentile=0.995)
    assert sampler._graph_key(thr, S, True, False, False, True) == ("dynthresh", 0.995, "dpm++", "pred_v", S, True)
    # the keys the plans of these diffusions ask for
    for gd, plan, want in ((v, sampler._plan_ancestral(v), (S, True)),
                           (mk("pred_v", sampling_timesteps=3), sampler._plan_ddim(mk("pred_v", sampling_timesteps=3)), (S, False)),
                           (thr, sampler._plan_dpm(thr), ("dynthresh", 0.995, "dpm++", "pred_v", S, True))):
        assert sampler._graph_key(gd, S, plan.with_noise, plan.rederive, False, plan.dpm) == want
