"""CPU: the launch trace and the host sequence of the training steps in ``lgm_hip.graph``.  The library is replaced by a
recorder (the pattern of tests/test_sampler_trace_host.py) and the stream / event / graph objects of ``torch.cuda`` by
fakes: a fake graph keeps the recorder calls made while it was being captured, a replay records itself.  The whole DDPM
step then runs on the CPU, and every case pins

  * the captured launches: the graphs' traces, in replay order, are the trace of one eager step of a twin up to its Adam
    launch - entry points, order and every scalar argument; pointers are left out - and each cut between two graphs falls
    right behind the last launch of an exchange bucket,
  * what ``step()`` does on the host: replays, ``ready`` per bucket range, ``finish``, the Adam launch(es), the EMA,
  * the memory pool every graph is captured into, the random stream around a capture, and the eager fallback when
    capture fails.

A further test pins what the first backward phase is the last holder of, for the four loss forms.  ``ModuleFastStep`` and
``WGANFastStep`` are driven with stub modules at the end of the file."""
import contextlib

import pytest
import torch

B = 2
KINDS = {"plain": dict(), "selfcond": dict(self_condition=True), "classes": dict(num_classes=3),
         "offset": dict(offset_noise_strength=0.1),
         # the other three loss forms: hybrid, weighted MSE and hybrid under a loss-aware timestep sampler (the *_iw entry points)
         "learned": dict(learned_variance=True), "tsampler": dict(t_sampler="loss_second_moment"),
         "learned_tsampler": dict(learned_variance=True, t_sampler="loss_second_moment")}
# layout -> (_ONE_GRAPH, _STEP_PIPELINE, with a gradient exchange, the bucket phases each graph holds)
WHOLE, HALVES, BUCKETS = ((0, 1, 2, 3),), ((0, 1), (2, 3)), ((0,), (1,), (2,), (3,))
LAYOUTS = {"one_graph": (True, False, False, WHOLE), "two_graphs": (False, False, False, HALVES),
           "sync": (True, False, True, BUCKETS), "pipeline": (True, True, False, BUCKETS),
           "pipeline_sync": (True, True, True, BUCKETS)}
FALLBACK = "[lgm_hip] HIP-graph capture unavailable (RuntimeError: no capture here); eager launches\n"


class _Recorder:
    """Stands in for the library: records (entry point, arguments) of every call and answers 0 (launched)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lgm_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Stream:
    def wait_stream(self, other):
        pass

    def wait_event(self, event):
        pass


class _Event:
    def record(self, stream=None):
        pass


class _Sync:
    """A gradient exchange that only records: ``ready(lo, hi)`` and ``finish()`` go into the recorder's list."""
    overlap = True
    grad_scale = 1.0

    def __init__(self, calls):
        self.calls = calls

    def ready(self, lo, hi):
        self.calls.append(("ready", (lo, hi)))

    def finish(self):
        self.calls.append(("finish", ()))


class _Session:
    def __init__(self, mp):
        from lgm_hip import graph, ops
        self.mp, self.graph, self.ops = mp, graph, ops
        self.rec = rec = _Recorder()
        self.captured = []                       # every fake graph, in capture order
        self.fail = False
        ses = self

        class Graph:
            def __init__(self):
                self.trace, self.kw = None, None

            def pool(self):                      # a graph captured into another graph's pool shares that pool
                return self.kw.get("pool", ("pool", id(self)))

            def replay(self):
                rec.calls.append(("replay", (id(self),)))

        @contextlib.contextmanager
        def capture(g, **kw):
            if ses.fail:
                raise RuntimeError("no capture here")
            g.kw, start = kw, len(rec.calls)
            yield
            g.trace = rec.calls[start:]
            ses.captured.append(g)

        mp.setattr(ops, "lib", lambda: rec)
        mp.setattr(ops, "stream", lambda: 0)
        cuda = torch.cuda
        mp.setattr(cuda, "is_current_stream_capturing", lambda: False)
        mp.setattr(cuda, "current_stream", lambda *a: _Stream())
        mp.setattr(cuda, "Stream", _Stream)
        mp.setattr(cuda, "stream", lambda s: contextlib.nullcontext())
        mp.setattr(cuda, "Event", _Event)
        mp.setattr(cuda, "synchronize", lambda *a: None)
        mp.setattr(cuda, "get_rng_state", lambda device=None: torch.get_rng_state())
        mp.setattr(cuda, "set_rng_state", lambda state, device=None: torch.set_rng_state(state))
        mp.setattr(cuda, "CUDAGraph", Graph)
        mp.setattr(cuda, "graph", capture)

    def ddpm(self, kind):
        from models.generative.diffusion.ddpm import DDPM
        torch.manual_seed(0)
        m = DDPM(img_channels=3, img_size=16, dim=16, diffusion_timesteps=10, ema_update_every=2, **KINDS[kind])
        m.sample_every = 0
        m.prepare_hip("cpu")
        m.train()
        g = torch.Generator().manual_seed(1)
        batch = (torch.rand(B, 3, 16, 16, generator=g) * 2 - 1, torch.tensor([0, 2]))
        return m, m.configure_optimizers(), batch

    def fast(self, kind, use_graph, with_sync, coins=()):
        m, opt, batch = self.ddpm(kind)
        fast = self.graph.DDPMFastStep(m, opt, 1, use_graph=use_graph)
        assert fast.sync is None and fast.mode == "eager" and fast.graphed is None and fast.net is m.ema.online_model.model
        if with_sync:
            fast.sync = _Sync(self.rec.calls)
        coins = iter(coins)
        fast.coin = lambda: next(coins)
        return fast, batch

    def run(self, fast, batch, idx):
        """one step -> the calls it recorded"""
        start = len(self.rec.calls)
        loss = fast.step(batch, idx)
        assert tuple(loss.shape) in ((), (1,)) and fast.model.logged["train_loss"] is loss
        return self.rec.calls[start:]

    def eager_steps(self, kind, with_sync, coins):
        """Steps 1 .. len(coins) of an eager twin.  Its step 0 is not looked at: it answers the plan queries and leaves
        gradients behind, as the warm-up in front of a capture does."""
        self.ops.clear_plan_caches()
        fast, batch = self.fast(kind, False, with_sync, (True,) + tuple(coins))
        self.run(fast, batch, 0)
        return fast, [self.run(fast, batch, i + 1) for i in range(len(coins))]


@pytest.fixture
def session(monkeypatch):
    return _Session(monkeypatch)


def _norm(calls):
    """entry points and scalar arguments; an address (or a ctypes object) becomes "ptr", a null pointer stays None"""
    def arg(a):
        if a is None or isinstance(a, (bool, float, str)) or (isinstance(a, int) and abs(a) < 1 << 32):
            return a
        return "ptr"
    return [(name, tuple(arg(a) for a in args)) for name, args in calls]


def _names(calls):
    return [name for name, _ in calls]


def _split(step, ranges):
    """An eager step with a recording exchange -> ([launches of bucket 0 (with the forward pass), 1, 2, 3], tail): the
    launches between the ``ready`` groups, which must be ``ranges``, and what follows the last group."""
    segs, got, cur, in_ready = [], [], [], False
    for c in step:
        if c[0] == "ready":
            if not in_ready:
                segs.append(cur)
                got.append([])
                cur, in_ready = [], True
            got[-1].append(c[1])
        else:
            cur.append(c)
            in_ready = False
    assert got == [list(r) for r in ranges] and len(segs) == 4
    return segs, cur


def _check_tail(tail, idx, total, with_sync):
    """finish, ONE Adam launch over the whole flat buffer, the EMA on the steps it updates (every second one here);
    ``idx``: the optimizer steps taken before this one"""
    names = _names(tail)
    if with_sync:
        assert names[0] == "finish"
        names, tail = names[1:], tail[1:]
    assert names[0] == "lgm_adam_step" and tail[0][1][4] == total and tail[0][1][10] == float(idx + 1)
    assert set(names[1:]) <= {"lgm_ema_lerp"} and (len(names) > 1) == (idx % 2 == 0)
    return names[1:]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_ddpm_step_trace(session, kind, layout):
    one_graph, pipeline, with_sync, groups = LAYOUTS[layout]
    graph = session.graph
    selfcond = kind == "selfcond"
    coins = (True, False, True)

    # ---- the eager twin: always with the recording exchange, whose ``ready`` calls mark the bucket boundaries
    twin, eager = session.eager_steps(kind, True, coins)
    net = twin.net
    ranges = net.bucket_ranges()
    total = net._flat.total
    flat = sorted(r for b in ranges for r in b)                          # the buckets tile the flat buffer
    assert flat[0][0] == 0 and flat[-1][1] == total and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
    split = [_split(s, ranges) for s in eager]
    for i, (segs, tail) in enumerate(split):
        _check_tail(tail, i + 1, total, True)
        assert _norm(sum(segs, [])) == _norm(sum(split[i % 2][0], []))     # a step's launches depend on the coin alone
    has_rows = [seg[-1][0] == "lgm_wgrad_reduce_batch" for seg in split[0][0]]
    if kind == "plain":
        assert sum(len(s) for s in split[1][0]) == 617
    # without an exchange the same launches, and nothing between them
    _, plain = session.eager_steps(kind, False, coins)
    for s, (segs, tail) in zip(plain, split):
        assert _norm(s) == _norm(sum(segs, []) + tail[1:])

    # ---- the graphed step
    session.mp.setattr(graph, "_ONE_GRAPH", one_graph)
    session.mp.setattr(graph, "_STEP_PIPELINE", pipeline)
    session.ops.clear_plan_caches()
    fast, batch = session.fast(kind, True, with_sync, coins)
    steps = [session.run(fast, batch, i) for i in range(3)]
    gs = fast.graphed
    assert fast.use_graph and gs is not None and isinstance(gs.graphs, list) and len(gs.graphs) == len(groups)
    assert (gs.pre is not None) == (gs.est is not None) == selfcond
    n = len(groups) + (1 if selfcond else 0)
    mode = ("hipGraph replay (4 graphs/step, weight passes on a side stream)" if pipeline else
            f"hipGraph replay ({n} graph{'s' if n > 1 else ''}/step)")
    if selfcond:
        mode = mode[:-1] + ", + the estimate graph on self-conditioned steps)"
    assert fast.mode == mode
    assert torch.equal(gs.x, batch[0]) and (gs.y is None) == (kind != "classes")
    assert kind != "classes" or torch.equal(gs.y, batch[1])

    # 1. captured launches
    def launches(seg):                           # the pipelined step launches the reductions itself, behind the replay
        return [c for c in seg if not (pipeline and c[0] == "lgm_wgrad_reduce_batch")]
    lead = ([gs.pre, gs.est] if selfcond else [])
    assert session.captured == lead + gs.graphs                          # capture order = replay order
    for coin, (segs, _) in zip((True, False), split):
        want = [launches(sum((segs[k] for k in group), [])) for group in groups]
        got = [g.trace for g in gs.graphs]
        head = (gs.pre.trace + (gs.est.trace if coin else [])) if selfcond else []
        assert _norm(head + got[0]) == _norm(want[0])
        for g, w in zip(got[1:], want[1:]):
            assert _norm(g) == _norm(w)
        assert sum(len(g) for g in got) + len(head) == sum(len(launches(s)) for s in segs)
    if selfcond:
        assert _names(gs.pre.trace) == ["lgm_qsample_target_slice"]
        assert _names(gs.est.trace)[-1] == "lgm_selfcond_estimate"
        assert "lgm_weighted_mse_fwd" not in _names(gs.est.trace)
    for g in gs.graphs[:-1]:                     # a cut falls behind a bucket's last launch: its batched reduction
        assert pipeline or g.trace[-1][0] == "lgm_wgrad_reduce_batch"

    # 2. the host sequence of every step (the capturing one: from its first replay on)
    first = _names(steps[0]).index("replay")
    assert "replay" not in _names(steps[0][:first])
    sync_ranges = [[r for k in group for r in ranges[k]] for group in groups]
    adam = split[0][1][1][1]                     # the twin's Adam arguments: its own step count apart, the same every step
    for i, (step, coin) in enumerate(zip([steps[0][first:]] + steps[1:], coins)):
        want = [("replay", (id(g),)) for g in (lead if coin else lead[:1])]
        it = iter(step[len(want):])
        assert step[:len(want)] == want
        for k, (g, rs) in enumerate(zip(gs.graphs, sync_ranges)):
            assert next(it) == ("replay", (id(g),))
            if pipeline and has_rows[k]:
                assert next(it)[0] == "lgm_wgrad_reduce_batch"
            if with_sync:
                for r in rs:
                    assert next(it) == ("ready", r)
            if pipeline:
                for lo, hi in rs:                # the bucket's slices of the Adam update
                    name, args = next(it)
                    assert name == "lgm_adam_step" and args[4] == hi - lo and args[10] == float(i + 1)
                    assert _norm([(name, args[5:10] + args[11:])]) == _norm([(name, adam[5:10] + adam[11:])])
        rest = list(it)
        if pipeline:
            assert not with_sync or _names(rest[:1]) == ["finish"]
            lerps = _names(rest[1:] if with_sync else rest)
            assert set(lerps) <= {"lgm_ema_lerp"} and (len(lerps) > 0) == (i % 2 == 0)
        else:
            lerps = _check_tail(rest, i, total, with_sync)
            args = rest[1 if with_sync else 0][1]
            assert _norm([("", args[:10] + args[11:])]) == _norm([("", adam[:10] + adam[11:])])

    # 3. every graph after the first is captured into the first one's pool
    head, *others = session.captured
    assert "pool" not in head.kw and head.kw == dict(capture_error_mode="thread_local")
    for g in others:
        assert g.kw == dict(capture_error_mode="thread_local", pool=("pool", id(head)))

    # what the last replay drew
    assert gs.t.shape == (B,) and gs.noise.shape == batch[0].shape and tuple(gs.loss.shape) == (1,)
    assert (gs.offset is not None) == (kind == "offset") and (gs.classes is not None) == (kind == "classes")
    assert net.grad_sync is None and getattr(net, "_flush_collect", None) is None


@pytest.mark.parametrize("kind", list(KINDS))
def test_capture_leaves_the_random_stream_alone(session, kind):
    m, opt, (x, y) = session.ddpm(kind)
    before = torch.get_rng_state()
    gs = session.graph.GraphedDDPMStep(m, opt, x.clone(), None, y=y if kind == "classes" else None)
    assert torch.equal(torch.get_rng_state(), before)
    calls = len(session.rec.calls)
    gs.step(0, True)
    assert _names(session.rec.calls[calls:])[-2:] == ["lgm_adam_step", "lgm_ema_lerp"]


@pytest.mark.parametrize("kind", ["plain", "selfcond"])
def test_failed_capture_falls_back_to_the_eager_step(session, kind, capsys):
    _, eager = session.eager_steps(kind, True, (True, False))
    session.fail = True
    session.ops.clear_plan_caches()
    fast, batch = session.fast(kind, True, True, (True, False))
    before = torch.get_rng_state()
    start = len(session.rec.calls)
    loss = fast.step(batch, 0)
    assert capsys.readouterr().err == FALLBACK
    assert fast.use_graph is False and fast.graphed is None and fast.mode == "eager" and tuple(loss.shape) == ()
    assert fast.net.grad_sync is None and getattr(fast.net, "_flush_collect", None) is None
    step = session.rec.calls[start:]
    assert "replay" not in _names(step)
    # the same call completes eagerly (entry points only: the accumulate flags of this one backward pass follow the
    # gradients the warm-up left behind)
    n = _names(eager[0]).index("lgm_adam_step")
    k = _names(step).index("lgm_adam_step")
    assert _names(step[k - n:k]) == _names(eager[0][:n])
    assert len(step) > k + 1 and set(_names(step[k + 1:])) == {"lgm_ema_lerp"}
    # the warm-up in front of the failed capture left the random stream alone: the eager step drew from ``before``
    after = torch.get_rng_state()
    torch.set_rng_state(before)
    twin, tbatch = session.fast(kind, False, True, (True,))
    torch.set_rng_state(before)
    session.run(twin, tbatch, 0)
    assert torch.equal(torch.get_rng_state(), after)
    again = session.run(fast, batch, 1)                                  # and it stays eager
    n = _names(eager[1]).index("lgm_adam_step")
    assert _norm(again[:n]) == _norm(eager[1][:n]) and _names(again[n:]) == ["lgm_adam_step"]
    assert capsys.readouterr().err == ""


LOSS_FORMS = {"mse": "plain", "mse_iw": "tsampler", "hybrid": "learned", "hybrid_iw": "learned_tsampler"}


def _tensors(saved):
    """every tensor in a nest of tuples and lists"""
    if torch.is_tensor(saved):
        return [saved]
    return [t for s in saved for t in _tensors(s)] if isinstance(saved, (tuple, list)) else []


@pytest.mark.parametrize("form", list(LOSS_FORMS))
def test_first_backward_phase_lets_go_of_what_it_alone_reads(session, form):
    """With the loss context gone, phase 0 of the backward pass (final conv, final block, up path) is the last holder of the
    final block's output, the output gradient, the network output, the target, the sampler's per-sample weights and what the
    up path saved: all of them are dead when it returns.  What the middle and the down path saved lives on for their phases."""
    import weakref
    from models.generative.diffusion import ddpm as D
    m, _, (x, _) = session.ddpm(LOSS_FORMS[form])
    gd = m.ema.online_model
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(2))
    _, ctx = D.hip_loss_forward(gd, x, torch.tensor([0, 9]), noise, True, True)
    assert (ctx.wb is not None) == form.endswith("_iw") and (ctx.per is not None) == form.startswith("hybrid")
    st = D.hip_loss_backward_begin(ctx, torch.ones(1))
    tape = ctx.tape
    later = _tensors([tape.time_saved, tape.downs, tape.sm1, tape.sm2, tape.sm3, tape.x])
    shared = {t.untyped_storage().data_ptr() for t in later}     # (the concat buffers: the down path wrote their skip halves)
    up = [t for t in _tensors([tape.ups, tape.final]) if t.untyped_storage().data_ptr() not in shared]
    assert len(up) > 20 and len(later) > 20
    dead = [weakref.ref(t) for t in [tape.fin, st.gout, ctx.out, ctx.target] + up + ([] if ctx.wb is None else [ctx.wb])]
    alive = [weakref.ref(t) for t in _tensors([tape.downs, tape.sm1, tape.sm2, tape.sm3])]
    del ctx, tape, later, up
    assert all(r() is not None for r in dead)
    gd.model.backward_run(st, 0, 0)
    assert [i for i, r in enumerate(dead) if r() is not None] == []
    assert all(r() is not None for r in alive)
    assert st.held is None and st.gout is None and st.fin is None and st.ups is None and st.final is None


# ---- ModuleFastStep / WGANFastStep on stub modules ------------------------------------------------------------------
class _Flat:
    def __init__(self):
        self.grad = torch.zeros(4)
        self.zeroed = 0

    def zero_grad(self):
        self.zeroed += 1


class _Opt:
    def __init__(self, owner=None):
        self.steps = self.zeroed = 0
        self.owner = owner

    def step(self):
        self.steps += 1
        if self.owner is not None:
            self.owner.global_step += 1          # what MiniTrainer's counting proxy does

    def zero_grad(self):
        self.zeroed += 1


class _Stub(torch.nn.Module):
    """``training_step``: a loss of the batch and the weight; it advances a buffer, counts a BatchNorm forward the way
    ``lgm_hip.bn`` does, draws from the generator and logs the loss."""

    def __init__(self):
        super().__init__()
        from lgm_hip.bn import BatchNorm2d
        self.w = torch.nn.Parameter(torch.ones(3))
        self.register_buffer("seen", torch.zeros(1))
        self.bn = BatchNorm2d(4)
        self.logged = {"kept": 1}
        self._flat = _Flat()
        self.ended = []

    def training_step(self, batch, batch_idx):
        from lgm_hip import bn
        x = batch[0]
        self.seen += 1
        with torch.no_grad():
            self.w.mul_(1.5)
        bn._count_forward(self.bn)
        loss = (self.w * x.mean() + 0 * torch.rand(3)).sum()
        self.logged["loss"] = loss.detach()
        return loss

    def on_train_batch_end(self, outputs, batch, batch_idx):
        self.ended.append(batch_idx)


def _state(m):
    return ([t.detach().clone() for t in list(m.parameters()) + list(m.buffers())], dict(m.logged), m.bn._nbt_pending,
            torch.get_rng_state())


def _same_state(m, state):
    tensors, logged, nbt, rng = state
    now = list(m.parameters()) + list(m.buffers())
    return (len(now) == len(tensors) and all(torch.equal(a, b) for a, b in zip(now, tensors)) and m.logged == logged
            and m.bn._nbt_pending == nbt and torch.equal(torch.get_rng_state(), rng))


def _replays(session, start=0):
    return [c for c in session.rec.calls[start:] if c[0] == "replay"]


def test_module_fast_step(session, capsys):
    graph = session.graph
    m, opt = _Stub(), _Opt()
    fast = graph.ModuleFastStep(m, opt, 1, True, False)
    assert fast.mode == "eager" and fast.static is None and fast.use_graph
    assert not graph.ModuleFastStep(m, opt, 2, True, True).use_graph     # a collective inside training_step: eager
    x = torch.full((2, 3), 2.0)
    before = _state(m)
    fast._capture((x, None))
    assert _same_state(m, before)                # capture = two warm-up runs + one captured: nothing of it is left
    assert fast.mode == "hipGraph replay (1 graph/step)" and len(session.captured) == 1
    assert isinstance(fast.static, tuple) and torch.equal(fast.static[0], x) and fast.static[0] is not x
    assert fast.static[1] is None

    # a batch of the captured shape: copied into the static input and replayed
    x2 = torch.full((2, 3), 5.0)
    loss = fast.step((x2, None), 7)
    assert _replays(session) == [("replay", (id(session.captured[0]),))]
    assert torch.equal(fast.static[0], x2)
    assert m.bn._nbt_pending == 1 and float(m.seen) == 0.0             # a fake replay runs nothing; the counter is the host's
    assert m.logged["kept"] == 1 and m.logged["loss"] is not None and loss is not None
    assert (opt.steps, opt.zeroed, m.ended) == (1, 1, [7])
    # another shape: eager
    loss = fast.step((torch.full((3, 3), 1.0), None), 8)
    assert len(_replays(session)) == 1 and float(m.seen) == 1.0 and m.bn._nbt_pending == 2
    assert float(loss.detach()) == pytest.approx(4.5) and m.w.grad is not None
    assert (opt.steps, opt.zeroed, m.ended) == (2, 2, [7, 8]) and m._flat.zeroed >= 1
    assert capsys.readouterr().err == ""


def test_module_fast_step_when_capture_fails(session, capsys):
    m, opt = _Stub(), _Opt()
    fast = session.graph.ModuleFastStep(m, opt, 1, True, False)
    session.fail = True
    before = _state(m)
    fast._capture((torch.full((2, 3), 2.0), None))
    assert capsys.readouterr().err == FALLBACK
    assert _same_state(m, before) and fast.use_graph is False and fast.mode == "eager"
    loss = fast.step((torch.full((2, 3), 2.0), None), 0)               # the step runs eagerly and does not try again
    assert float(loss.detach()) == pytest.approx(9.0) and float(m.seen) == 1.0 and not _replays(session)
    assert (opt.steps, m.ended) == (1, [0]) and capsys.readouterr().err == ""


class _Hp:
    n_critic = 2


class _Gen(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.g = torch.nn.Parameter(torch.ones(3))
        self._flat = _Flat()

    def random_sample(self, n):
        return self.g * torch.rand(n, 3)


class _Gan(_Stub):
    hparams = _Hp

    def __init__(self):
        super().__init__()
        self.G, self.D = _Gen(), _Gen()
        self.global_step = 0
        self.log = []

    def _loss(self, key, value):
        from lgm_hip import bn
        self.seen += 1
        bn._count_forward(self.bn)
        return {key: value.sum(), "aux": float(self.seen)}

    def _calculate_d_loss(self, x, x_hat):
        return self._loss("d_loss", (x - x_hat) * self.D.g)

    def _calculate_g_loss(self, x_hat):
        return self._loss("g_loss", x_hat)

    def log_dict(self, logs, **kw):
        self.log.append(set(logs))


def test_wgan_fast_step(session, capsys):
    m = _Gan()
    opts = (_Opt(m), _Opt(m))
    fast = session.graph.WGANFastStep(m, opts, 1, True)
    assert fast.mode == "eager" and fast.graphs == {} and fast.sync is None
    x = torch.full((2, 3), 2.0)
    seq = []
    for i in range(6):                           # n_critic = 2: critic, critic, generator, ...
        before = _state(m)
        captures = len(session.captured)
        logs = fast.step((x + i, None), i)
        seq.append("d" if "d_loss" in logs else "g")
        if len(session.captured) > captures:     # this step captured its graph: bump aside, the state is as before
            assert m.bn._nbt_pending == before[2] + 1
            m.bn._nbt_pending -= 1
            assert _same_state(m, before)
            m.bn._nbt_pending += 1
        if i == 0:
            assert set(fast.graphs) == {"d"}
    assert seq == ["d", "d", "g", "d", "d", "g"] and m.log == [{"d_loss", "aux"}] * 2 + [{"g_loss", "aux"}] + \
        [{"d_loss", "aux"}] * 2 + [{"g_loss", "aux"}]
    assert set(fast.graphs) == {"d", "g"} and len(session.captured) == 2
    assert fast.mode == "hipGraph replay (critic graph / generator graph)"
    d, g = session.captured
    assert [c[1][0] for c in _replays(session)] == [id(d), id(d), id(g), id(d), id(d), id(g)]
    assert (opts[0].steps, opts[1].steps, m.global_step, m.bn._nbt_pending) == (4, 2, 6, 6)
    assert float(m.seen) == 0.0                  # every step was a (fake) replay
    # another shape runs eagerly, on the schedule's key
    n = len(_replays(session))
    logs = fast.step((torch.ones(3, 3), None), 6)
    assert "d_loss" in logs and len(_replays(session)) == n and float(m.seen) == 1.0 and m.D._flat.zeroed >= 1
    # ``_capture(key, x)`` is what the benchmark calls up front
    fast2 = session.graph.WGANFastStep(_Gan(), opts, 1, True)
    for key in ("d", "g"):
        fast2._capture(key, x)
    assert set(fast2.graphs) == {"d", "g"}
    assert capsys.readouterr().err == ""


def test_wgan_fast_step_when_capture_fails(session, capsys):
    m = _Gan()
    fast = session.graph.WGANFastStep(m, (_Opt(m), _Opt(m)), 1, True)
    session.fail = True
    before = _state(m)
    fast._capture("d", torch.ones(2, 3))
    assert capsys.readouterr().err == FALLBACK
    assert _same_state(m, before) and fast.use_graph is False and fast.graphs == {} and fast.mode == "eager"
    assert "d_loss" in fast.step((torch.ones(2, 3), None), 0) and not _replays(session) and float(m.seen) == 1.0
