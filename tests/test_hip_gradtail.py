"""GPU: the gradient tail - lgm_grad_sqnorm_partial / lgm_grad_clip_scale / lgm_adam_step_scaled / lgm_grad_accumulate
(csrc/optim.hip), FusedAdam(max_grad_norm), gradient accumulation on the graph-replayed step objects and MiniTrainer's
``accumulate_grad_batches`` / ``gradient_clip_val`` - against the float64 references of tests/gradtail_ref.py at the tolerance
fixed on the CPU by tests/test_gradtail_host.py.

Flat operands live inside NaN-filled buffers with 32 elements of guard on both sides, as in tests/test_hip_streaming.py;
guards and the tail behind element n must stay NaN.  Every score goes through the ``parity`` fixture."""
import math

import pytest
import torch

import gradtail_ref as gr
from oracle import streaming as st
from oracle.bounds import forward_error_units

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


class Flat:
    """n elements inside a NaN buffer: 32 elements of guard in front, at least four NaN behind element n - 1 and the rear guard"""

    def __init__(self, data, dev, n=None, dtype=torch.float32):
        self.n = n = data.numel() if data is not None else n
        self.buf = torch.full((GUARD + (n + 3) // 4 * 4 + 4 + GUARD,), NAN, device=dev, dtype=dtype)
        self.view = self.buf[GUARD:GUARD + n]
        if data is not None:
            self.view.copy_(data.to(dev))

    def result(self):
        return self.view.detach().cpu().clone()

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.n:]).all())


def _span():
    from lgm_hip import ops
    return ops.grad_sqnorm_span(1)


def _clip_scale(dev, grads, grad_scale, max_norm):
    """partial pass over every gradient into ONE workspace, then one lgm_grad_clip_scale -> (out2 Flat, partials Flat)"""
    from lgm_hip import ops
    counts = [ops.grad_sqnorm_partials(g.n) for g in grads]
    partials = Flat(None, dev, n=sum(counts), dtype=torch.float64)
    out2 = Flat(None, dev, n=2)
    off = 0
    for g, c in zip(grads, counts):
        ops.grad_sqnorm_partial(g.view, partials.view[off:off + c])
        off += c
    ops.grad_clip_scale(partials.view, grad_scale, max_norm, out2.view)
    torch.cuda.synchronize()
    assert partials.intact() and out2.intact() and all(g.intact() for g in grads), "a guard or a NaN tail was written"
    return out2, partials


def _rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


# ---- 1. the norm ------------------------------------------------------------------------------------------------------------------

def _norm_sizes():
    span = _span()
    return list(st.FLAT_SIZES) + [span - 1, span, span + 1, 3 * span + 5]


def test_sqnorm_and_clip_scale(dev, parity):
    """out2[1] against the float64 norm: at most 2^-24 + n 2^-53 relative; the partial sums, read back as doubles: at most
    n 2^-53; the clipped scale: the same bound as the norm it is formed from; guards intact; two runs give equal bits"""
    from lgm_hip import ops
    grad_scale, max_norm = 0.125, 2.0 ** -10                # both cross the ABI as floats: exact ones
    for n in _norm_sizes():
        g = st.adam_inputs(n, 2)[1]
        gf = Flat(g, dev)
        out2, partials = _clip_scale(dev, [gf], grad_scale, max_norm)
        assert partials.n == ops.grad_sqnorm_partials(n) == -(-n // _span())
        assert st.exact_units(gf.result(), g) == 0.0, "the gradient is read-only"
        ssum, want = math.fsum(partials.result().tolist()), gr.sqnorm64(g)
        parity(f"sqnorm n={n}: sum of the partials, relative", _rel(ssum, want), n * 2.0 ** -53 + 1e-300)
        scale, norm = gr.clip_scale64(g, grad_scale, max_norm)
        got = out2.result()
        parity(f"sqnorm n={n}: norm, relative", _rel(float(got[1]), norm), gr.norm_bound(n))
        if scale != grad_scale:                                                  # the clip acts (at every size but the smallest)
            parity(f"sqnorm n={n}: clipped scale, relative", _rel(float(got[0]), scale), gr.norm_bound(n) + 2.0 ** -50)
        else:
            assert n < 1023 and float(got[0]) == grad_scale
        again, partials2 = _clip_scale(dev, [Flat(g, dev)], grad_scale, max_norm)
        assert torch.equal(partials2.result().view(torch.int64), partials.result().view(torch.int64)), n
        assert st.exact_units(again.result(), got) == 0.0, f"n={n}: two runs differ"


def test_partials_of_two_buffers_give_the_norm_of_their_concatenation(dev, parity):
    span = _span()
    g1, g2 = st.adam_inputs(span + 1, 2)[1], st.adam_inputs(1027, 7)[1]
    out2, partials = _clip_scale(dev, [Flat(g1, dev), Flat(g2, dev)], 1.0, 1.0)
    assert partials.n == 3
    both = torch.cat([g1, g2])
    scale, norm = gr.clip_scale64(both, 1.0, 1.0)
    got = out2.result()
    parity("two buffers: norm, relative", _rel(float(got[1]), norm), gr.norm_bound(both.numel()))
    parity("two buffers: scale, relative", _rel(float(got[0]), scale), gr.norm_bound(both.numel()) + 2.0 ** -50)


def test_zero_inf_and_nan_gradients(dev):
    n = _span() + 5
    zero = _clip_scale(dev, [Flat(torch.zeros(n), dev)], 0.125, 1.0)[0].result()
    assert float(zero[0]) == 0.125 and float(zero[1]) == 0.0, "all-zero gradients: the scale is grad_scale exactly"
    g = st.adam_inputs(n, 2)[1]
    for where in (0, n - 1):                                  # a whole span and the tail
        bad = g.clone()
        bad[where] = float("inf")
        got = _clip_scale(dev, [Flat(bad, dev)], 0.125, 1.0)[0].result()
        assert float(got[0]) == 0.0 and math.isinf(float(got[1])), "one inf element: coefficient 0"
        bad[where] = float("nan")
        got = _clip_scale(dev, [Flat(bad, dev)], 0.125, 1.0)[0].result()
        assert math.isnan(float(got[0])) and math.isnan(float(got[1])), "one NaN element: a NaN scale, as torch's clamp gives"


@pytest.mark.parametrize("n", [5, 1024, 1027, 3074])
def test_grad_accumulate_is_torchs_sum(dev, n):
    from lgm_hip import ops
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    dst, src = Flat(a, dev), Flat(b, dev)
    ops.grad_accumulate(dst.view, src.view)
    torch.cuda.synchronize()
    assert dst.intact() and src.intact() and st.exact_units(dst.result(), a + b) == 0.0
    ops.grad_accumulate(dst.view, src.view, overwrite=True)
    torch.cuda.synchronize()
    assert dst.intact() and src.intact() and st.exact_units(dst.result(), b) == 0.0 and st.exact_units(src.result(), b) == 0.0


# ---- 2. the clipped Adam kernel -----------------------------------------------------------------------------------------------------

def _run_clipped_adam(case, dev, plain=False):
    """partials -> scale -> lgm_adam_step_scaled from the case's state (plain: lgm_adam_step at the case's grad_scale)"""
    from lgm_hip import ops
    hp = case.hp
    p, g, m, v = (Flat(t, dev) for t in case.inputs)
    args = (p.view, g.view, m.view, v.view, case.n, hp["lr"], hp["betas"][0], hp["betas"][1], st.ADAM_EPS, hp["wd"], case.step,
            None)
    if plain:
        ops.adam_step(*args, hp["grad_scale"], hp["decoupled"])
    else:
        out2, _ = _clip_scale(dev, [g], hp["grad_scale"], case.max_norm)
        ops.adam_step_scaled(*args, out2.view, hp["decoupled"])
    torch.cuda.synchronize()
    assert all(f.intact() for f in (p, g, m, v)), f"{case.name}: a guard or the NaN tail behind element n was written"
    assert st.exact_units(g.result(), case.inputs[1]) == 0.0, "the gradient is read-only"
    return {"p": p.result(), "m": m.result(), "v": v.result()}


def _judge(parity, case, got):
    for k, units in case.scores(got).items():
        parity(f"{case.name}: {k}", units, case.tol)


ADAM_SIZES = (1, 3, 4, 5, 1027, 3074)


@pytest.mark.parametrize("config", gr.CLIP_CONFIGS)
def test_adam_step_scaled(dev, parity, config):
    """p, m and v of one clipped step against adam_formula in float64 at grad_scale * coef, max_norm 1 and 1e-3; with
    max_norm 1e6 the coefficient is 1 and the bits are those of a plain lgm_adam_step from the same state"""
    for n in ADAM_SIZES:
        for step in gr.CLIP_STEPS:
            for max_norm in (1.0, 1e-3):
                case = gr.ClipCase(n, config, step, max_norm)
                _judge(parity, case, _run_clipped_adam(case, dev))
            case = gr.ClipCase(n, config, step, 1e6)
            assert case.scale == case.hp["grad_scale"]
            got, plain = _run_clipped_adam(case, dev), _run_clipped_adam(case, dev, plain=True)
            for k in got:
                assert st.exact_units(got[k], plain[k]) == 0.0, f"{case.name}: {k} differs from the plain kernel"


def test_adam_step_scaled_where_the_1e_6_shows(dev, parity):
    for n in ADAM_SIZES:
        for step in gr.CLIP_STEPS:
            case = gr.ClipCase(n, "ddpm", step, gr.TINY_MAX_NORM, grad_scale=gr.TINY_SCALE)
            _judge(parity, case, _run_clipped_adam(case, dev))


# ---- the DDPM module ----------------------------------------------------------------------------------------------------------------

B = 8


def _ddpm(dev, seed=10):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(seed)
    m = DDPM(img_channels=3, img_size=16, dim=16, lr=1e-3)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


def _flat(m):
    return m.ema.online_model.model._flat


def _batches(dev, n, seed=8):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, 16, 16, generator=g) * 2 - 1).to(dev) for _ in range(n)]


def _hp(opt):
    grp = opt.param_groups[0]
    return dict(lr=grp["lr"], betas=grp["betas"], wd=grp["weight_decay"], decoupled=grp["decoupled"], eps=grp["eps"])


def _judge_step(parity, what, before, after, grad, step, hp, grad_scale, max_norm, norm_got):
    """one optimizer step over a whole flat buffer against the float64 reference: the norm within the bound of test 1, p, m
    and v within the tolerance of test 2"""
    n = grad.numel()
    scale, norm = gr.clip_scale64(grad, grad_scale, max_norm)
    parity(f"{what}: norm, relative", _rel(float(norm_got), norm), gr.norm_bound(n))
    ref, S = st.adam_formula(before["p"], grad, before["m"], before["v"], step, grad_scale=scale, **hp)
    for k in ("p", "m", "v"):
        parity(f"{what}: {k}", forward_error_units(after[k], ref[k], S[k]), gr.tolerance())
    return scale, norm


def _state(opt, fp):
    st_ = opt._flat_state.get(id(fp))
    zeros = torch.zeros(fp.total)
    return {"p": fp.data.cpu().clone(), "m": st_["m"].cpu().clone() if st_ else zeros, "v": st_["v"].cpu().clone() if st_ else zeros}


def test_fused_adam_clips_the_ddpm_step(dev, parity):
    """FusedAdam(max_grad_norm=1.0), three eager steps: norm, p, m and v of every step within the bounds of the kernel tests
    on the whole flat buffer; a twin without clipping ends elsewhere"""
    a, b = _ddpm(dev), _ddpm(dev)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    oa.max_grad_norm = 1.0
    fa, fb = _flat(a), _flat(b)
    g = torch.Generator().manual_seed(4)
    clipped = 0
    for i, x in enumerate(_batches(dev, 3)):
        t = torch.randint(0, 1000, (B,), generator=g).to(dev)
        noise = torch.randn(B, 3, 16, 16, generator=g).to(dev)
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m.ema.online_model.p_losses(x, t, noise, _normalize=True).backward()
        before, grad = _state(oa, fa), fa.grad.cpu().clone()
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        scale, norm = _judge_step(parity, f"step {i + 1}", before, _state(oa, fa), grad, i + 1, _hp(oa), 1.0, 1.0,
                                  oa.last_grad_norm)
        clipped += scale < 1.0
        assert st.exact_units(fa.grad.cpu(), grad) == 0.0, "the gradient is read-only"
    assert clipped, "max_grad_norm = 1 never acted"
    assert not torch.equal(fa.data, fb.data)
    assert ob.last_grad_norm is None and oa.last_grad_norm.device.type == "cuda" and oa.last_grad_norm.dim() == 0
    ws = oa._clip_ws[0].data_ptr()
    oa.step()
    assert oa._clip_ws[0].data_ptr() == ws, "nothing is allocated after the first clipped step"


# ---- 4. accumulation ----------------------------------------------------------------------------------------------------------------

class _Run:
    """``n`` micro-batches through DDPMFastStep(accumulate=K); ``entry`` holds the flat gradient on entry of every optimizer
    step, ``scales`` the optimizer's grad_scale there.  With ``twin`` the micro-gradients ``micro`` come from a twin's eager
    p_losses + backward on the draws the step made, and the twin then takes the optimizer step on their sequential sum."""

    def __init__(self, dev, K, n, use_graph=True, clip=None, twin=False, sync=None, flush=False):
        from lgm_hip.graph import DDPMFastStep
        from lgm_hip.lightning import _CountingOptimizer
        self.model = a = _ddpm(dev)
        self.opt = oa = a.configure_optimizers()
        oa.max_grad_norm = clip
        a._optimizers = [_CountingOptimizer(oa, a)]
        self.fast = fast = DDPMFastStep(a, a._optimizers[0], 1, use_graph=use_graph, accumulate=K)
        if sync is not None:
            fast.sync = sync(_flat(a))
        self.entry, self.scales, self.norms, self.micro = [], [], [], []
        fa, step = _flat(a), oa.step

        def recording_step(*args, **kw):
            self.entry.append(fa.grad.clone())
            self.scales.append(oa.grad_scale)
            out = step(*args, **kw)
            if oa.last_grad_norm is not None:
                self.norms.append(oa.last_grad_norm.clone())
            return out
        oa.step = recording_step
        if twin:
            b = _ddpm(dev)
            ob, fb, gd_b = b.configure_optimizers(), _flat(b), b.ema.online_model
            assert torch.equal(fa.data, fb.data)
        torch.manual_seed(77)                                  # the device generator: the same draws in every run
        for i, x in enumerate(_batches(dev, n)):
            if sync is not None:
                fast.sync.micro = i
            fast.step((x.clone(), None), i)
            if twin:
                ob.zero_grad()
                gd_b.p_losses(x, fast.graphed.t.clone(), fast.graphed.noise.clone(), _normalize=True).backward()
                self.micro.append(fb.grad.clone())
                b.on_train_batch_end(None, None, i)
                if (i + 1) % K == 0:
                    fb.grad.copy_(gr.accumulate_sum(self.micro[-K:]))
                    ob.grad_scale = oa.grad_scale
                    ob.step()
                    assert torch.equal(fa.data, fb.data), f"optimizer step {(i + 1) // K}: the twin's parameters differ"
        if flush:
            fast.flush()
        torch.cuda.synchronize()

    def state(self):
        fa = _flat(self.model)
        s = self.opt._flat_state[id(fa)]
        return dict(p=fa.data, m=s["m"], v=s["v"], ema=self.model.ema.ema_model.model._flat.data, step=s["step"])


@pytest.fixture(scope="module")
def graph_run(dev):
    """K = 3, six micro-batches, graph replay, with the twin: shared by the accumulation tests below"""
    return _Run(dev, 3, 6, twin=True)


def test_accumulated_gradient_is_the_sequential_sum(graph_run):
    """(a) on entry of each optimizer step the flat gradient is (g1 + g2) + g3 of the three micro-gradients, bit for bit"""
    r = graph_run
    assert r.fast.mode.startswith("hipGraph") and r.fast.graphed.pipeline is False
    assert len(r.entry) == 2 and r.scales == [1.0 / 3, 1.0 / 3]
    for j in range(2):
        assert torch.equal(r.entry[j], gr.accumulate_sum(r.micro[3 * j:3 * j + 3])), f"optimizer step {j + 1}"
        assert not torch.equal(r.entry[j], r.micro[3 * j + 2])
    assert r.fast.accum.k == 0 and r.fast.accum.acc.data_ptr() != _flat(r.model).grad.data_ptr()


def test_accumulation_graph_replay_equals_eager_launches(dev, graph_run):
    """(b) the same object from eager launches: equal parameters, moments and EMA shadow; two optimizer steps"""
    e = _Run(dev, 3, 6, use_graph=False)
    assert e.fast.mode == "eager" and graph_run.fast.mode.startswith("hipGraph")
    assert e.model.global_step == graph_run.model.global_step == 2
    sg, se = graph_run.state(), e.state()
    assert sg["step"] == se["step"] == 2
    for k in ("p", "m", "v", "ema"):
        assert torch.equal(sg[k], se[k]), k
    for a, b in zip(graph_run.entry, e.entry):
        assert torch.equal(a, b)


def test_clipped_norm_is_the_norm_of_the_accumulated_mean(dev, parity, graph_run):
    """(c) accumulation and clipping together: last_grad_norm is the float64 norm of (g1 + g2 + g3) / 3"""
    r = _Run(dev, 3, 3, clip=1.0)
    assert len(r.entry) == 1 and torch.equal(r.entry[0], graph_run.entry[0])        # the same draws, the same weights
    _, norm = gr.clip_scale64(r.entry[0], 1.0 / 3, 1.0)
    parity("K = 3: norm of the mean, relative", _rel(float(r.norms[0]), norm), gr.norm_bound(r.entry[0].numel()))
    assert not torch.equal(r.state()["p"], _Run(dev, 3, 3).state()["p"]) or norm <= 1.0


def test_flush_steps_on_what_is_pending(dev, graph_run):
    """(d) five micro-batches, then flush(): two optimizer steps, the second over two micro-gradients at scale 1/3"""
    r = _Run(dev, 3, 5, flush=True)
    assert r.model.global_step == 2 and len(r.entry) == 2 and r.scales == [1.0 / 3, 1.0 / 3]
    assert torch.equal(r.entry[0], graph_run.entry[0])
    assert torch.equal(r.entry[1], gr.accumulate_sum(graph_run.micro[3:5]))
    assert r.fast.accum.k == 0
    r.fast.flush()                                            # nothing pending: nothing happens
    assert r.model.global_step == 2


def test_module_fast_step_accumulates(dev):
    """(e) ModuleFastStep on the small VQ-VAE at K = 2 with a batch of another shape in the middle: the gradient on entry of
    each optimizer step is g1 + g2 of a twin's eager micro-gradients, and the parameters follow"""
    from lgm_hip.graph import ModuleFastStep
    from models.generative.vae.vqvae import VQVAE

    def make():
        torch.manual_seed(5)
        m = VQVAE(img_channels=3, img_size=32, embedding_dim=64, num_embeddings=512, hidden_dim=64,
                  num_residual_layers=2, num_residual_hiddens=32, use_ema=True, lr=1e-3, b1=0.9, b2=0.999,
                  loss_weights={"recon_loss": 1, "vq_loss": 10}).to(dev)
        m.prepare_hip(dev)
        m.train()
        return m, m.configure_optimizers()

    (a, oa), (b, ob) = make(), make()
    fa = a.make_fast_step(oa, 1, True, accumulate=2)
    assert isinstance(fa, ModuleFastStep)
    tb = ModuleFastStep(b, ob, 1, use_graph=False)             # the twin: its forward + backward only
    entry, step = [], oa.step

    def recording_step(*args, **kw):
        entry.append(a._flat.grad.clone())
        return step(*args, **kw)
    oa.step = recording_step
    g = torch.Generator().manual_seed(8)
    micro = []
    for i, Bx in enumerate((64, 64, 24, 64, 64)):
        x = (torch.rand(Bx, 3, 32, 32, generator=g) * 2 - 1).to(dev)
        fa.step((x, None), i)
        tb._fwd_bwd((x.clone(), None), i)
        micro.append(b._flat.grad.clone())
        b.on_train_batch_end(None, None, i)
        if i % 2 == 1:
            assert len(entry) == (i + 1) // 2 and torch.equal(entry[-1], micro[-2] + micro[-1]), i
            b._flat.grad.copy_(micro[-2] + micro[-1])
            ob.grad_scale = 0.5
            ob.step()
            ob.zero_grad()
            assert torch.equal(a._flat.data, b._flat.data), i
    assert fa.mode.startswith("hipGraph") and len(entry) == 2 and oa.grad_scale == 0.5
    fa.flush()                                                # the fifth micro-batch alone, at scale 1/2
    assert len(entry) == 3 and torch.equal(entry[2], micro[4]) and oa.grad_scale == 0.5


# ---- 5. one exchange per optimizer step, overlapped ---------------------------------------------------------------------------------

class _RecordingSync:
    """FlatGradSync's surface.  ``ready(lo, hi)`` copies flat.grad[lo:hi] into a snapshot on the current stream: what a
    collective enqueued there would read."""
    world, overlap = 2, True

    def __init__(self, flat):
        self.flat, self.calls, self.finished, self.micro = flat, [], [], 0
        self.snapshot = torch.full_like(flat.grad, NAN)

    @property
    def grad_scale(self):
        return 1.0 / self.world

    def ready(self, lo, hi):
        self.calls.append((self.micro, lo, hi))
        self.snapshot[lo:hi].copy_(self.flat.grad[lo:hi])
        return None

    def finish(self):
        self.finished.append(self.micro)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_one_exchange_per_optimizer_step(dev, use_graph):
    K = 3
    r = _Run(dev, K, K, use_graph=use_graph, twin=use_graph, sync=_RecordingSync)
    stub, total = r.fast.sync, _flat(r.model).total
    if use_graph:
        assert len(r.fast.graphed.graphs) == 4, "with an exchange the step is cut where a bucket becomes final"
    assert all(micro == K - 1 for micro, _, _ in stub.calls), "ready() on a micro-step that does not end in an optimizer step"
    assert stub.finished == [K - 1]
    spans, at = sorted((lo, hi) for _, lo, hi in stub.calls), 0
    for lo, hi in spans:
        assert lo == at and hi > lo, "the calls of step K cover the buffer once"
        at = hi
    assert at == total
    assert torch.equal(stub.snapshot, r.entry[0])
    if use_graph:
        assert torch.equal(stub.snapshot, gr.accumulate_sum(r.micro))
    assert r.scales == [1.0 / (K * stub.world)] and r.opt.grad_scale == 1.0 / (K * stub.world)


# ---- 6. the trainer -----------------------------------------------------------------------------------------------------------------

def _fit(dev, n, fast_path):
    from lgm_hip.lightning import MiniTrainer
    m = _ddpm(dev)
    data = [(x.cpu(), torch.zeros(B, dtype=torch.long)) for x in _batches(dev, n)]
    tr = MiniTrainer(max_epochs=1, accumulate_grad_batches=2, gradient_clip_val=1.0, log_every=0, device=dev, fast_path=fast_path)
    torch.manual_seed(77)
    tr.fit(m, train_dataloader=data)
    torch.cuda.synchronize()
    return m, tr


def test_trainer_accumulates_and_clips_on_the_fast_path(dev, parity):
    """MiniTrainer(accumulate_grad_batches=2, gradient_clip_val=1.0), five batches: the fast step in graph mode, three
    optimizer steps.  One optimizer step from equal state against the slow path (which accumulates inside the backward
    kernels with beta = 1 and rounds in another order): within the tolerance of the clipped Adam kernel, in units of the
    float64 reference's companion for the fast path's own gradient.  The distance after all five batches is put on record."""
    from lgm_hip.graph import DDPMFastStep
    fast, tr = _fit(dev, 5, True)
    assert isinstance(tr.fast, DDPMFastStep) and tr.fast.mode.startswith("hipGraph")
    assert fast.global_step == 3
    assert fast._optimizers[0].max_grad_norm == 1.0 and fast._optimizers[0].grad_scale == 0.5
    assert float(fast._optimizers[0].last_grad_norm) > 0 and "grad_norm" not in fast.logged       # read only at log time
    slow, trs = _fit(dev, 5, False)
    assert trs.fast is None and slow.global_step == 3
    pf, ps = _flat(fast).data.cpu(), _flat(slow).data.cpu()
    parity.record("five batches, fast path against slow path", max_abs=float((pf - ps).abs().max()),
                  rel_l2=float((pf - ps).double().norm() / ps.double().norm()))
    # one optimizer step (two micro-batches) from equal state
    p0 = _flat(_ddpm(dev)).data.cpu().clone()
    one_f, trf = _fit(dev, 2, True)
    one_s, _ = _fit(dev, 2, False)
    assert one_f.global_step == one_s.global_step == 1
    opt = one_f._optimizers[0]
    grad = _flat(one_f).grad.cpu().clone()                     # the accumulated sum the fast path stepped on
    scale, _ = gr.clip_scale64(grad, 0.5, 1.0)
    zeros = torch.zeros_like(p0)
    ref, S = st.adam_formula(p0, grad, zeros, zeros, 1, grad_scale=scale, **_hp(opt))
    pf, ps = _flat(one_f).data.cpu(), _flat(one_s).data.cpu()
    parity("one step, fast path against the float64 reference: p", forward_error_units(pf, ref["p"], S["p"]), gr.tolerance())
    parity("one step, fast path against slow path: p", forward_error_units(pf, ps.double(), S["p"]), gr.tolerance())
