"""GPU: the timestep samplers of the diffusion training step (``GaussianDiffusion(t_sampler=...)``, lgm_hip/tsampler.py).

  * lgm_tsampler_update against tests/tsampler_ref.py: the rows EXACTLY (values are copied, not computed; L_b of a
    learned-variance network is one float32 product and one float32 sum, restated in float32), in the smallest batches at
    which the ordering can go wrong; the plan (cdf, iw, and p = 1 / (T iw)) against float64 from the same float32 history at
    1e-4 relative - a fixed-order float32 sum of T <= 1000 non-negative terms is off by at most (T - 1) 2^-24 ~ 6e-5, the square
    root and the divides add a few roundings.
  * lgm_tsampler_draw bit for bit against numpy (searchsorted on the float32 cdf; the stratified draw in float32).
  * the weighted loss and its gradient at the network output against the float64 restatement mean_b(iw[t_b] L_b): L_b and
    dL_b / dout are the plain kernels' (bounded against float64 at 1e-4 by tests/test_hip_ops.py and
    tests/test_hip_learned_sigma.py), so the bound here is that 1e-4 plus one rounding, 2^-24, for the extra multiply; with
    iw = 1 (not warm) loss and gradient equal the "uniform" model's bit for bit.
  * the whole step, graph replay against eager launches, bit for bit, state included; "uniform" draws what a model built
    without the keyword draws; eval mode records nothing; a checkpoint round trip continues the run."""
import numpy as np
import pytest
import torch

import tsampler_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-4
H = 10
Q = 0.001
ONE_BELOW = float(np.nextafter(np.float32(1), np.float32(0)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _lib():
    from lgm_hip import ops
    return ops.lib(), ops.stream()


def _last():
    from lgm_hip import ops
    return ops.lib()._dll.lgm_last_kernel().decode()


def _update(dev, state, t, per, vb_weight=0.0, q=Q):
    """one lgm_tsampler_update launch on the arrays of ``state`` -> (history, counts, cdf, iw) as numpy"""
    L, st = _lib()
    h, c = state.arrays()
    hd, cd = torch.as_tensor(h).to(dev), torch.as_tensor(c).to(dev)
    guard = torch.full((state.T + 2,), float("nan"), device=dev)         # cdf between two guard values
    cdf, iw = guard[1:-1], torch.full((state.T,), float("nan"), device=dev)
    B = 0 if t is None else len(t)
    td = None if t is None else torch.as_tensor(np.asarray(t, np.int64)).to(dev)
    pd = None if per is None else torch.as_tensor(np.asarray(per, np.float32)).to(dev).contiguous()
    n_terms = 1 if per is None or np.asarray(per).ndim == 1 else 2
    L.lgm_tsampler_update(None if td is None else td.data_ptr(), None if pd is None else pd.data_ptr(), n_terms,
                          float(vb_weight), hd.data_ptr(), cd.data_ptr(), state.H, float(q), state.T, B, cdf.data_ptr(),
                          iw.data_ptr(), st)
    assert _last() == "tsampler_update_kernel"
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard[0])) and bool(torch.isnan(guard[-1])), "the update wrote outside cdf"
    return hd.cpu().numpy(), cd.cpu().numpy(), cdf.cpu().numpy(), iw.cpu().numpy()


def _rows_equal(hist, counts, state):
    assert counts.dtype == np.int32 and counts.tolist() == state.counts.tolist()
    for t, row in enumerate(state.rows):
        got = hist[t, :len(row)]
        assert got.tolist() == [float(v) for v in row], f"row {t}: {got.tolist()} != {[float(v) for v in row]}"


def _warm(rng, T, decades=6.0, rows=H):
    return R.State(T, H, [(10.0 ** rng.uniform(-decades, 0.0)) * (0.5 + np.abs(rng.standard_normal(rows))) for _ in range(T)])


# ---- the update kernel: rows ------------------------------------------------------------------------------------------------
def _ordering_cases(T):
    rng = np.random.default_rng(T)
    mid = T // 2
    st = _warm(rng, T)
    st.rows[mid] = st.rows[mid][:9]                           # count 9: the first of three fills the row, the others wrap
    yield "fills and wraps inside one batch", st, [mid, 1, mid, 3, mid, 1, 2, 5], np.arange(1, 9, dtype=np.float32)
    st = R.State(T, H)
    st.rows[mid] = [np.float32(-1), np.float32(-2)]
    yield "B = 12, all equal: the last 10 survive", st, [mid] * 12, np.arange(1, 13, dtype=np.float32)
    st = _warm(rng, T)
    st.rows[2] = st.rows[2][:4]
    yield ("NaN and +inf are not recorded", st, [2, 2, 2, 4, 4, 2, 0, 2],
           np.array([1, np.nan, 2, np.inf, 3, -np.inf, np.nan, 4], np.float32))
    st = R.State(T, H)
    yield "t = 0 and t = T - 1", st, [0, T - 1, 0, T - 1, T - 1, 0, T - 1, 0], np.arange(1, 9, dtype=np.float32)


def test_update_rows_of_a_batch_staged_in_two_rounds(dev):
    """B = 1030 > the 1024 samples one staging round holds: rows fill, wrap and keep their order across the rounds"""
    T = 16
    rng = np.random.default_rng(1030)
    st = R.State(T, H)
    t, L = rng.integers(0, T, 1030), np.arange(1, 1031, dtype=np.float32)
    L[[5, 1024, 1027]] = np.nan
    hist, counts, _, _ = _update(dev, st, t, L)
    st.update(t, L)
    _rows_equal(hist, counts, st)
    assert st.warm() and max(max(map(float, r)) for r in st.rows) == 1030.0


# T = 2500: more rows than the workgroup has threads (a thread owns up to three)
@pytest.mark.parametrize("T", [16, 1000, 2500])
def test_update_rows_against_reference(dev, T):
    for what, st, t, L in _ordering_cases(T):
        hist, counts, cdf, iw = _update(dev, st, t, L)
        st.update(t, L)
        _rows_equal(hist, counts, st)
        p, cdf64, iw64, weighted = R.plan(st, Q)                          # the plan belongs to the UPDATED rows
        assert np.all(np.abs(cdf - cdf64) <= RTOL * cdf64), what
        assert np.all(np.abs(iw - iw64) <= RTOL * iw64), what
    # a learned-variance batch: L_b = per[0][b] + vb_weight per[1][b] in float32; timesteps outside the table are skipped
    rng = np.random.default_rng(7)
    st = _warm(rng, T)
    per = np.stack([rng.uniform(0.01, 1.0, 8), rng.uniform(0.1, 30.0, 8)]).astype(np.float32)
    t = [3, 3, T - 1, 0, T, -1, 3, 1]
    hist, counts, _, _ = _update(dev, st, t, per, vb_weight=0.001)
    st.update(t, R.per_sample_loss(per, 0.001))
    _rows_equal(hist, counts, st)


# ---- the update kernel: plan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 1000, 2500])
def test_plan_against_float64(dev, parity, T):
    """(T = 2500, a thread owns up to three rows: the kernel's sums are two-level - at most 3 + 6 + 16 roundings in sum(w), two
    runs of 50 in the prefix sum - so the bound derived for a plain sum of 1000 terms holds there as well)"""
    import json
    import os
    rng = np.random.default_rng(100 + T)
    worst = {}

    def check(what, st, q=Q):
        hist, counts, cdf, iw = _update(dev, st, None, None, q=q)
        _rows_equal(hist, counts, st)                                     # an empty batch changes no row
        p, cdf64, iw64, weighted = R.plan(st, q)
        assert cdf.dtype == np.float32 and cdf[-1] == np.float32(1.0) and np.all(np.diff(cdf) >= 0) and cdf[0] >= 0
        e_cdf = float(np.max(np.abs(cdf - cdf64) / cdf64))
        e_iw = float(np.max(np.abs(iw - iw64) / iw64))
        e_p = float(np.max(np.abs(1.0 / (T * iw.astype(np.float64)) - p) / p))
        for k, e in (("cdf", e_cdf), ("iw", e_iw), ("p = 1 / (T iw)", e_p)):
            worst[f"{what}: {k}"] = parity(f"T = {T}, {what}: {k} against float64, relative", e, RTOL) / RTOL
        return cdf, iw, weighted

    _, iw, weighted = check("rows over six decades", _warm(rng, T))
    assert weighted and iw.min() < 0.5 and iw.max() > 2.0, "the history was to give a non-uniform plan"
    st = _warm(rng, T)
    st.rows[T // 3] = [np.float32(0)] * H
    _, iw, weighted = check("one zero row", st, q=0.01)
    assert weighted and abs(iw[T // 3] - 100.0) <= RTOL * 100.0, "p_t = q / T on a zero row"
    st = _warm(rng, T)
    st.rows[T - 1] = st.rows[T - 1][:H - 1]
    _, iw, weighted = check("not warm (one row one short)", st)
    assert not weighted and np.all(iw == np.float32(1.0)), "not warm: iw = 1.0 exactly"
    _, iw, weighted = check("warm, every row zero", R.State(T, H, [np.zeros(H)] * T))
    assert not weighted and np.all(iw == np.float32(1.0))
    _, iw, _ = check("empty", R.State(T, H))
    assert np.all(iw == np.float32(1.0))
    path = os.environ.get("LGM_TSAMPLER_PARITY")
    if path:                                                              # the committed copy: profiles/r16_tsampler_parity.json
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[f"T={T}"] = {"bound": RTOL, "worst_ratio": max(worst.values()), "ratios": worst}
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)


# ---- the draw kernel --------------------------------------------------------------------------------------------------------
def _draw(dev, u, cdf, T, mode, B):
    L, st = _lib()
    ud = torch.as_tensor(np.asarray(u, np.float32)).to(dev)
    cd = None if cdf is None else torch.as_tensor(np.asarray(cdf, np.float32)).to(dev)
    guard = torch.full((B + 2,), -7, dtype=torch.long, device=dev)
    L.lgm_tsampler_draw(ud.data_ptr(), None if cd is None else cd.data_ptr(), T, mode, guard[1:].data_ptr(), B, st)
    assert _last() == "tsampler_draw_kernel"
    torch.cuda.synchronize()
    assert int(guard[0]) == -7 and int(guard[-1]) == -7, "the draw wrote outside t"
    return guard[1:-1].cpu().numpy()


@pytest.mark.parametrize("T", [16, 1000])
def test_cdf_draw_is_searchsorted(dev, T):
    rng = np.random.default_rng(T)
    # a cdf the kernel built, and one with flat runs (zero-probability timesteps, also the first and the last)
    _, _, built, _ = _update(dev, _warm(rng, T), None, None)
    p = rng.uniform(0.0, 1.0, T)
    p[[0, 1, T // 2, T // 2 + 1, T - 1]] = 0.0
    flat = np.cumsum(p / p.sum()).astype(np.float32)
    flat[-2:] = 1.0
    for cdf in (built, flat):
        u = np.concatenate([[0.0, ONE_BELOW, np.nextafter(np.float32(cdf[0]), np.float32(2))], cdf[:-1][cdf[:-1] < 1.0][:: max(1, T // 16)],
                            np.nextafter(cdf[T // 2], np.float32(0))[None], rng.uniform(0, 1, 8)]).astype(np.float32)
        u = u[u < 1.0]
        want = R.cdf_draw(cdf, u)
        got = _draw(dev, u, cdf, T, 1, len(u))
        assert got.dtype == np.int64 and got.tolist() == want.tolist()
        assert got.tolist() == np.minimum(T - 1, np.searchsorted(cdf, u, side="right")).tolist()
        assert np.all(cdf[got] > u), "the drawn timestep has probability mass above u"
        got8 = _draw(dev, u[:8], cdf, T, 1, 8)
        assert got8.tolist() == want[:8].tolist()


@pytest.mark.parametrize("B", [8, 12])
@pytest.mark.parametrize("u0", [0.0, ONE_BELOW, 0.37])
def test_stratified_draw_is_the_float32_restatement(dev, B, u0):
    T = 1000
    got = _draw(dev, [u0], None, T, 0, B)
    want = R.stratified_draw(u0, B, T)
    assert got.tolist() == want.tolist()
    assert got.min() >= 0 and got.max() <= T - 1 and len(set(got.tolist())) == B
    assert _draw(dev, [u0], None, 16, 0, B).tolist() == R.stratified_draw(u0, B, 16).tolist()


# ---- loss and gradient -------------------------------------------------------------------------------------------------------
S, DIM, B = 16, 16, 8


def _diffusion(dev, T, learned, t_sampler="loss_second_moment", seed=3):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    torch.manual_seed(seed)
    net = Unet(dim=DIM, channels=3, **(dict(learned_variance=True) if learned else {}))
    kw = dict(vb_loss_weight=0.01) if learned else {}
    gd = GaussianDiffusion(net, img_size=S, timesteps=T, objective="pred_noise", beta_schedule="cosine", t_sampler=t_sampler,
                           **kw).to(dev)
    net.prepare_hip(dev)
    return gd.train()


def _batch(dev, T):
    g = torch.Generator().manual_seed(T)
    img, noise = torch.rand(B, 3, S, S, generator=g), torch.randn(B, 3, S, S, generator=g)
    t = torch.tensor([0, 1, T // 2, T // 2, T - 1, 3, 0, T - 2])
    return img.to(dev), t.to(dev), noise.to(dev)


def _loss_and_gout(gd, img, t, noise):
    from models.generative.diffusion import ddpm as D
    gd.model._flat.zero_grad()
    loss, ctx = D.hip_loss_forward(gd, img, t, noise, True, True)
    st = D.hip_loss_backward_begin(ctx, torch.ones(1, device=img.device))
    gout = st.gout.clone()
    gd.model.backward_run(st)
    torch.cuda.synchronize()
    return loss.clone(), gout, ctx


@pytest.mark.parametrize("learned", [False, True], ids=["mse", "hybrid"])
@pytest.mark.parametrize("T", [16, 1000])
def test_weighted_loss_and_gradient(dev, parity, T, learned):
    img, t, noise = _batch(dev, T)
    plain = _diffusion(dev, T, learned, "uniform")
    loss_u, gout_u, ctx_u = _loss_and_gout(plain, img, t, noise)
    gd = _diffusion(dev, T, learned)
    ts = gd._ts
    # not warm: the plain kernels' bits, and the batch is recorded
    loss_n, gout_n, _ = _loss_and_gout(gd, img, t, noise)
    assert torch.equal(loss_n, loss_u) and torch.equal(gout_n, gout_u), "iw = 1: loss and gradient are the plain kernels'"
    assert int(ts.counts.sum()) == B and int(ts.counts[0]) == 2 and int(ts.counts[T // 2]) == 2
    # warm and non-uniform
    rng = np.random.default_rng(T + learned)
    st = _warm(rng, T, decades=3.0)
    h, c = st.arrays()
    ts.load_state(h, c)
    ts.ensure_plan()
    iw_dev = ts.iw.cpu().numpy().copy()
    loss_w, gout_w, ctx = _loss_and_gout(gd, img, t, noise)
    p, cdf64, iw64, weighted = R.plan(st, ts.q)
    assert weighted and iw64[t.cpu().numpy()].max() / iw64[t.cpu().numpy()].min() > 2.0
    # L_b: the unweighted per-sample terms the plain forward left, in float64
    if learned:
        per = ctx_u.per.double().cpu().numpy()
        assert torch.equal(ctx.per, ctx_u.per), "the history records the unweighted terms"
        L64 = per[0] + gd.vb_loss_weight * per[1]
        L32 = R.per_sample_loss(ctx_u.per.cpu().numpy(), gd.vb_loss_weight)
    else:
        out, target = ctx_u.out.double().cpu(), ctx_u.target.double().cpu()
        mse = ((out[..., :3] - target[..., :3]) ** 2).mean(dim=(1, 2, 3)).numpy()
        L64 = gd.loss_weight.double().cpu().numpy()[t.cpu().numpy()] * mse
        L32 = None
    tn = t.cpu().numpy()
    want, dl = R.weighted_loss(iw64, tn, L64)
    bound = RTOL + 2.0 ** -24
    parity(f"T = {T}: weighted loss against mean_b(iw[t_b] L_b) in float64", abs(float(loss_w) - want) / abs(want), bound)
    assert abs(want - float(np.mean(L64))) > 10 * RTOL * abs(want), "the weights were to move the loss"
    wb = torch.as_tensor(iw64[tn]).reshape(B, 1, 1, 1)
    g_want = gout_u.double().cpu() * wb
    e = float((gout_w.double().cpu() - g_want).norm() / g_want.norm())
    parity(f"T = {T}: output gradient against iw[t_b] dL_b / dout in float64", e, bound)
    for b in range(B):
        e = float((gout_w[b].double().cpu() - g_want[b]).norm() / g_want[b].norm())
        parity(f"T = {T}: output gradient of sample {b} (t = {int(tn[b])})", e, bound)
    assert torch.equal(ctx.wb.cpu(), torch.as_tensor(iw_dev)[t.cpu()]), "wb = iw[t_b] of the plan the step drew from"
    # the step recorded the UNWEIGHTED losses behind the loss, and the plan now belongs to the updated rows
    if L32 is None:                                           # (per [B] is not kept: the rows' newest entries against L_b)
        once = [1, 4, 5, 7]                                   # the samples whose timestep the batch holds once
        got = np.array([ts.history[int(tb), -1].item() for tb in tn[once]])
        assert np.all(np.abs(got - L64[once]) <= RTOL * L64[once])
    else:
        st.update(tn, L32)
        _rows_equal(ts.history.cpu().numpy(), ts.counts.cpu().numpy(), st)
    assert not torch.equal(ts.iw.cpu(), torch.as_tensor(iw_dev))
    # the public path: p_losses with an explicit t weights the same way (the state has moved on: same plan reloaded)
    ts.load_state(h, c)
    again = gd.p_losses(img, t, noise, _normalize=True)
    assert torch.equal(again.detach().reshape(1), loss_w)
    # eval mode: unweighted, nothing recorded
    before = (ts.history.clone(), ts.counts.clone())
    gd.eval()
    with torch.no_grad():
        ev = gd.p_losses(img, t, noise, _normalize=True)
    assert torch.equal(ev.reshape(1), loss_u) and torch.equal(ts.history, before[0]) and torch.equal(ts.counts, before[1])


# ---- the whole step ----------------------------------------------------------------------------------------------------------
def _module(dev, T=16, seed=10, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(seed)
    m = DDPM(img_size=S, dim=DIM, lr=1e-3, diffusion_timesteps=T, beta_schedule="cosine", objective="pred_noise", **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


def _preload(m, T, seed=5):
    st = _warm(np.random.default_rng(seed), T, decades=3.0)
    m.ema.online_model._ts.load_state(*st.arrays())


def _record_draws(ts):
    seen, orig = [], ts.draw

    def draw(n, device):
        t = orig(n, device)
        seen.append(t)
        return t
    ts.draw = draw
    return seen


@pytest.mark.parametrize("variant", ["plain", "accumulate", "learned", "stratified"])
def test_graph_replay_equals_eager_launches(dev, variant):
    T = 16
    kw = dict(learned_variance=True, vb_loss_weight=0.01) if variant == "learned" else {}
    kw["t_sampler"] = "stratified" if variant == "stratified" else "loss_second_moment"
    acc = 2 if variant == "accumulate" else 1
    a, b = _module(dev, T, **kw), _module(dev, T, **kw)
    if variant != "stratified":
        _preload(a, T), _preload(b, T)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True, accumulate=acc), b.make_fast_step(ob, 1, False, accumulate=acc)
    tsa, tsb = a.ema.online_model._ts, b.ema.online_model._ts
    graph_t, eager_t = [], _record_draws(tsb)
    g = torch.Generator().manual_seed(1)
    xs = [torch.rand(B, 3, S, S, generator=g).to(dev) for _ in range(5 * acc)]       # 5 optimizer steps
    before = a.ema.online_model.model._flat.data.clone()
    for fast in (fa, fb):
        torch.manual_seed(77)
        for i, x in enumerate(xs):
            fast.step((x.clone(), None), i)
            if fast is fa:
                graph_t.append(fa.graphed.t.clone())
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    assert len(graph_t) == len(eager_t) == len(xs)
    for i, (tg, te) in enumerate(zip(graph_t, eager_t)):
        assert torch.equal(tg, te), f"step {i}: t of the replay {tg.tolist()} and of eager launches {te.tolist()}"
    if variant != "stratified":
        assert len({tuple(tg.tolist()) for tg in graph_t}) > 1
        for k in ("history", "counts", "cdf", "iw"):
            assert torch.equal(getattr(tsa, k), getattr(tsb, k)), f"{k}: graph replay and eager launches differ"
        assert int(tsa.counts.min()) == H and bool(torch.isfinite(tsa.history).all())
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data), "parameters: graph replay and eager launches differ"
    assert not torch.equal(na._flat.data, before) and bool(torch.isfinite(na._flat.data).all())


def test_capture_leaves_the_sampler_state_alone(dev):
    """warm-up and capture run the step several times: the rows, the counts and the plan are put back"""
    T = 16
    a = _module(dev, T, t_sampler="loss_second_moment")
    ts = a.ema.online_model._ts
    fa = a.make_fast_step(a.configure_optimizers(), 1, True)
    x = torch.rand(B, 3, S, S).to(dev)
    torch.manual_seed(5)
    fa.step((x, None), 0)
    assert fa.mode.startswith("hipGraph")
    assert int(ts.counts.sum()) == B, "one step, one batch recorded"
    t = fa.graphed.t.cpu().numpy()
    per_row = np.bincount(t, minlength=T)
    assert ts.counts.cpu().numpy().tolist() == per_row.tolist()


def test_uniform_draws_what_a_model_without_the_keyword_draws(dev):
    a, b = _module(dev, 1000, t_sampler="uniform"), _module(dev, 1000)
    fa, fb = a.make_fast_step(a.configure_optimizers(), 1, True), b.make_fast_step(b.configure_optimizers(), 1, True)
    g = torch.Generator().manual_seed(2)
    xs = [torch.rand(B, 3, S, S, generator=g).to(dev) for _ in range(3)]
    drawn = []
    for fast in (fa, fb):
        torch.manual_seed(123)
        for i, x in enumerate(xs):
            fast.step((x.clone(), None), i)
            drawn.append((fast.graphed.t.clone(), fast.graphed.noise.clone()))
    torch.manual_seed(123)
    t0 = torch.randint(0, 1000, (B,), device=dev).long()
    assert torch.equal(drawn[0][0], t0), "the first draw of the step is the reference's randint"
    for (ta, na), (tb, nb) in zip(drawn[:3], drawn[3:]):
        assert torch.equal(ta, tb) and torch.equal(na, nb)
    assert fa.graphed.ts is None and a.ema.online_model._ts is None
    assert torch.equal(a.ema.online_model.model._flat.data, b.ema.online_model.model._flat.data)


def test_eval_mode_records_nothing(dev):
    T = 16
    m = _module(dev, T, learned_variance=True, t_sampler="loss_second_moment")
    _preload(m, T)
    ts = m.ema.online_model._ts
    ts.ensure_plan()
    before = [getattr(ts, k).clone() for k in ("history", "counts", "cdf", "iw")]
    x = torch.rand(4, 3, S, S).to(dev)
    m.eval()
    with torch.no_grad():
        m.validation_step((x, None))
        bpd = m.bits_per_dim(x)
    assert bool(torch.isfinite(bpd).all()) and "val_loss" in m.logged
    for k, v in zip(("history", "counts", "cdf", "iw"), before):
        assert torch.equal(getattr(ts, k), v), f"{k} changed in eval mode"
    # the online model itself in eval mode: a uniform draw, nothing recorded
    gd = m.ema.online_model
    with torch.no_grad():
        gd(x)
    assert torch.equal(ts.history, before[0]) and torch.equal(ts.counts, before[1])
    m.train()
    assert gd.active_t_sampler() is ts


def test_checkpoint_round_trip(dev, tmp_path):
    from lgm_hip.lightning import save_checkpoint
    T = 16
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand(B, 3, S, S, generator=g).to(dev) for _ in range(4)]

    def run(m, fast, steps, first):
        for i in range(first, first + steps):
            torch.manual_seed(1000 + i)
            fast.step((xs[i].clone(), None), i)
        ts = m.ema.online_model._ts
        return fast.graphed.t.clone(), ts.history.clone(), ts.counts.clone(), ts.cdf.clone()

    a = _module(dev, T, t_sampler="loss_second_moment")
    _preload(a, T)                                            # warm: every draw depends on the rows
    oa = a.configure_optimizers()
    fa = a.make_fast_step(oa, 1, True)
    run(a, fa, 3, 0)
    path = str(tmp_path / "last.ckpt")
    save_checkpoint(a, [oa], path)
    want = run(a, fa, 1, 3)
    ckpt = torch.load(path, map_location=dev, weights_only=False)
    assert "ema.online_model.t_sampler.history" in ckpt["state_dict"] and "ema.online_model.t_sampler.counts" in ckpt["state_dict"]
    assert ckpt["hyper_parameters"]["t_sampler"] == "loss_second_moment"
    b = _module(dev, T, seed=99, t_sampler="loss_second_moment")
    b.load_state_dict(ckpt["state_dict"])
    b.prepare_hip(dev)
    ob = b.configure_optimizers()
    ob.load_state_dict(ckpt["optimizer_states"][0])
    fb = b.make_fast_step(ob, 1, True)
    got = run(b, fb, 1, 3)
    for k, w, g_ in zip(("t", "history", "counts", "cdf"), want, got):
        assert torch.equal(w, g_), f"{k} of the 4th step: the resumed run differs from the uninterrupted one"
    assert int(got[2].min()) == H and not torch.equal(got[3], torch.linspace(1 / T, 1, T, device=dev))
