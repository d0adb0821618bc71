"""HIP-graph replay of the training steps.

At small per-GPU batches (strong scaling: 128 / N images per GPU) the ~400 kernel launches of a DDPM step are
host-bound when issued from Python.  The step is therefore captured ONCE and replayed (GraphedDDPMStep).  The UNet's
backward pass runs in four phases, each of which makes one exchange bucket of the flat gradient buffer final
(``Unet.BACKWARD_PHASES`` / ``bucket_ranges()``); a LAYOUT says which phases share a graph:

    one rank : ((0, 1, 2, 3),)            ONE graph - t ~ randint (or the diffusion's timestep sampler: its draw here, its
                                          state update behind the loss, lgm_hip.tsampler), noise ~ randn (a diffusion with offset
                                          noise also draws its [B, C] offsets, a class-conditional one its label drop), q_sample,
                                          UNet forward, loss, the whole backward - then fused Adam (1 eager kernel) and
                                          EMA (every 10th step);  ``LGM_ONE_GRAPH=0``: ((0, 1), (2, 3))
    N ranks  : ((0,), (1,), (2,), (3,))   FOUR graphs, cut where a bucket becomes final, with the asynchronous
                                          all-reduce of each bucket issued between the replays

Collectives are never captured, the optimiser's step count lives on the host, and the RNG is torch's graph-safe
Philox generator.  The arithmetic is identical to the eager path (same kernels, same order) - tested bit for bit.
ModuleFastStep (VQ-VAE: one graph), WGANFastStep (critic graph / generator graph) and GANFastStep (the MLP GAN: the work in
front of and behind the D optimizer step, two graphs on one memory pool) follow the same rules and keep
what they captured in a ``_Captured``: warm-up and capture leave the training state untouched (_TrainingState), also
when capture fails.  Every step class falls back to eager launches when capture is not possible (``_eager_fallback``).
``accumulate > 1`` (DDPMFastStep, ModuleFastStep) leaves the captured graphs as they are: the micro-gradients are summed in one
extra flat buffer behind the replays and the exchange, the norm and Adam run once per K micro-steps (``_GradAccumulation``).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .captured import _warm_up
from .lightning import multi_rank


import os as _os
import random

_ONE_GRAPH = _os.environ.get("LGM_ONE_GRAPH", "1") == "1"           # one rank: the whole step in ONE graph (A/B switch)
_STEP_PIPELINE = _os.environ.get("LGM_STEP_PIPELINE", "0") == "1"   # opt-in: weight passes of a bucket on a side stream


class _TrainingState:
    """Everything a warm-up / capture run of a training step may advance and a run that never tried to capture
    would not have: parameters and buffers (EMA codebooks, running statistics), the device random stream, the
    host-side BatchNorm batch counters and what the module logged.  ``restore()`` is called from a ``finally``: a
    capture that FAILS leaves the same state behind as one that succeeds, so the eager fallback is identical to a
    run that was eager from the start."""

    def __init__(self, modules, device):
        from .bn import BatchNorm2d
        self.device = device
        self.tensors = []
        seen = set()
        for m in modules:
            for t in list(m.parameters()) + list(m.buffers()):
                if id(t) not in seen:
                    seen.add(id(t))
                    self.tensors.append(t)
        self.snap = [t.detach().clone() for t in self.tensors]
        self.bns = [b for m in modules for b in m.modules() if isinstance(b, BatchNorm2d)]
        self.nbt = [b._nbt_pending for b in self.bns]
        self.logged = [(m, dict(m.logged)) for m in modules if hasattr(m, "logged")]
        self.rng = torch.cuda.get_rng_state(device)

    def restore(self):
        with torch.no_grad():
            for t, s in zip(self.tensors, self.snap):
                t.copy_(s)
        for b, n in zip(self.bns, self.nbt):
            b._nbt_pending = n
        for m, lg in self.logged:
            m.logged.clear()
            m.logged.update(lg)
        torch.cuda.set_rng_state(self.rng, self.device)


def _capture(fn, warmup: int, pool=None):
    """Eager warm-up of ``fn``, then its capture into a HIP graph.  Returns (graph, fn's return value inside the capture,
    BatchNorm modules whose train-mode forward ran inside it — a replay does not pass through Python, so the step
    object advances their host-side batch counters itself).  thread_local: only THIS thread is held to the capture
    rules — the RCCL watchdog thread of a multi-GPU job keeps polling its events while the step is being captured."""
    from . import bn
    _warm_up(fn, warmup)
    g = torch.cuda.CUDAGraph()
    bn.CAPTURE_TRACE = []
    try:
        kw = dict(capture_error_mode="thread_local")
        if pool is not None:
            kw["pool"] = pool
        with torch.cuda.graph(g, **kw):
            out = fn()
        trace = bn.CAPTURE_TRACE
    finally:
        bn.CAPTURE_TRACE = None
    return g, out, trace


def _eager_fallback(step, e: Exception):
    """Capture is an optimisation: when it is not possible the step object goes on with eager launches."""
    import sys
    print(f"[lgm_hip] HIP-graph capture unavailable ({type(e).__name__}: {e}); eager launches", file=sys.stderr, flush=True)
    step.use_graph = False


class _Captured:
    """One captured function of a training step: its graph, the static inputs a batch is copied into, what the function
    returned inside the capture (tensors in the graph's memory: every replay refreshes them in place) and the BatchNorm
    modules whose forward ran inside."""

    def __init__(self, graph, static, out, bn_trace):
        self.graph, self.static, self.out, self.bn_trace = graph, static, out, bn_trace

    @classmethod
    def of(cls, fn, batch, modules, device):
        """Capture ``fn(static copy of batch)``.  Whatever warm-up and capture did to the training state is undone, on
        success and when capture raises."""
        static = tuple(b.clone() if torch.is_tensor(b) else b for b in batch)
        state = _TrainingState(modules, device)
        try:
            g, out, trace = _capture(lambda: fn(static), 2)
        finally:
            state.restore()
        return cls(g, static, out, trace)

    def matches(self, batch) -> bool:
        return all((not torch.is_tensor(b)) or b.shape == s.shape for b, s in zip(batch, self.static))

    def replay(self, batch):
        for b, s in zip(batch, self.static):
            if torch.is_tensor(b):
                s.copy_(b)
        self.graph.replay()
        for b in self.bn_trace:                      # BatchNorm forwards inside the graph: host-side batch counters
            b._nbt_pending += 1
        return self.out


class _GradAccumulation:
    """``accumulate_grad_batches = K > 1`` over one flat gradient buffer.  The backward passes (captured or eager) go on
    overwriting ``flat.grad``; this object owns the ONE extra buffer ``acc`` and counts micro-steps.  Micro-step k of K:

        k = 1 < K   ``stash``: acc = grad           no exchange, no optimizer step
        1 < k < K   ``stash``: acc += grad          no exchange, no optimizer step
        k = K       ``fold``:  grad += acc          (slice by slice, in front of that slice's exchange), then the tail
                                                    of a plain step: exchange, norm, Adam - all of them read ``flat.grad``

    so the stepped gradient is the sequential float32 sum ((g1 + g2) + ...) + gK, and ``scale()`` = base / K is the
    mean over micro-batches that Lightning's ``loss / K`` gives, folded into Adam like 1 / world."""

    def __init__(self, flat, K: int):
        self.flat, self.K, self.k = flat, int(K), 0      # k: micro-gradients held in ``acc``
        self.acc = torch.empty_like(flat.grad)

    @property
    def stepping(self) -> bool:
        """the micro-step now running is the Kth: its tail ends in the optimizer step"""
        return self.k == self.K - 1

    def scale(self, base: float) -> float:
        return base / self.K

    def stash(self):
        ops.grad_accumulate(self.acc, self.flat.grad, overwrite=self.k == 0)
        self.k += 1

    def fold(self, lo: int, hi: int):
        if self.k:
            ops.grad_accumulate(self.flat.grad[lo:hi], self.acc[lo:hi])

    def unstash(self):
        """``flush``: the pending sum becomes the gradient (no micro-gradient of this step exists)"""
        ops.grad_accumulate(self.flat.grad, self.acc, overwrite=True)
        self.k = 0                                       # nothing left to fold

    def stepped(self):
        self.k = 0


def _accumulated_step(opt, sync, accum: _GradAccumulation):
    """The end of the Kth micro-step and of ``flush``.  Without an exchange nothing has read the gradient yet: ONE add
    over the whole buffer.  Then the optimizer step at 1 / (K world) and a new sum."""
    if sync is None:
        accum.fold(0, accum.flat.total)
    else:
        sync.finish()
    getattr(opt, "_opt", opt).grad_scale = accum.scale(sync.grad_scale if sync is not None else 1.0)
    opt.step()
    accum.stepped()


def _clipping(opt) -> bool:
    return bool(getattr(getattr(opt, "_opt", opt), "clipping", False))


LAYOUT_ONE, LAYOUT_TWO, LAYOUT_BUCKETS = ((0, 1, 2, 3),), ((0, 1), (2, 3)), ((0,), (1,), (2,), (3,))


class GraphedDDPMStep:
    """The DDPM step as graphs.  ``self.layout`` holds, per graph, the backward phases (= exchange buckets) it runs:

        phase 0  backward of final block + up path          -> bucket 0 [ups], [final]
        phase 1  backward of the middle blocks              -> bucket 1 [mid]
        phase 2  backward of the down path + init conv      -> bucket 2 [init, downs]
        phase 3  backward of the time MLP / FiLM projections -> bucket 3 [FiLM, time]

    The first graph opens with t, noise, q_sample, UNet forward, loss and the loss gradient.  One rank: ``LAYOUT_ONE``,
    one Adam launch (``LGM_ONE_GRAPH=0``: ``LAYOUT_TWO`` - no measurable difference).  With a gradient exchange (``sync``):
    ``LAYOUT_BUCKETS``, so that each bucket's all-reduce is issued the moment its slice is final and runs beside
    everything that follows it; ``self.ranges[i]`` are the flat-buffer slices final after graph i.

    ``LGM_STEP_PIPELINE=1`` (opt-in, measured SLOWER on one GPU: 11.69 vs 11.44 ms at B = 128, 4.77 vs 4.65 ms at
    B = 16): ``LAYOUT_BUCKETS`` on every rank count, and behind each graph on a SIDE stream the bucket's weight-sized passes -
    batched slab reduction, all-reduce, ITS slice of the Adam update (a bucket's weights are not read again by the
    backward once its gradients are final).  Bit-identical to the default (tested), but the streaming kernels' workgroups
    delay the one-workgroup-per-CU convolutions more than the overlap returns, and two more graph boundaries plus five
    Adam slices cost 0.2 ms by themselves.  Kept for multi-GPU experiments, where the Adam slices would run beside the
    later buckets' all-reduces.

    Self-conditioned model (reference :899-909): whether a step runs the estimate pass is a HOST coin, so the first graph is cut
    behind the launch that draws t / noise and writes x_t (``pre``), the estimate pass - the network without saved
    activations + the kernel that writes x_start into the self-conditioning slice of the input buffer - is a graph of its own
    (``est``) replayed on the steps whose coin says so, and the saved forward pass opens the next graph.  ``pre`` zeroes the
    self-conditioning slice on every step.  A model without self-conditioning captures exactly the graphs of its layout.

    Class-conditional model: ``y`` is a second static input buffer (the batch's labels, copied beside ``x`` before replay).
    The label drop of classifier-free guidance - rand(B) < cond_drop_prob - is drawn inside the graph behind t, noise and
    offset, the order ``GaussianDiffusion.forward`` draws in.  A model without classes draws nothing more.

    ``self.t`` / ``self.noise`` / ``self.offset`` (the [B, C] offset noise of a diffusion with ``offset_noise_strength > 0``)
    / ``self.classes`` hold what the last replay drew.

    Dropout (``Unet(dropout=p)``, p > 0): the step's 64-bit key is drawn inside the graph behind every other draw, into the
    diffusion's persistent ``dropout_key`` tensor (``self.dropout_key``); the GroupNorm launches of the forward and of the
    backward graphs read it from the device, so every replay - every accumulation micro-step - runs under its own key.  A
    self-conditioned model draws it in ``pre``; its estimate pass is pass 1 of the mask.  p == 0: nothing is drawn.

    Low-resolution conditioned model (``Unet(lowres_cond=True)``): the augmentation levels s ~ randint(0, lowres_aug_levels) and
    the augmentation noise are drawn inside the graph behind every other draw (``self.lowres_s`` / ``self.lowres_noise``), and
    the launch that writes the conditioning slice from the batch follows q_sample's.  Any other model draws nothing more.

    The protocol (``models.generative.diffusion.ddpm.Diffusion``).  Every diffusion rides this step through the two methods its
    eager ``forward`` goes through: ``draw(x, labels) -> StepDraws``, the one place its draw order is written, and
    ``qsample(x, draws, normalize) -> QSample``, its launches up to the input buffer and the target.  The record is left in
    ``self.t`` / ``self.noise`` / ``self.offset`` / ``self.classes`` / ``self.dropout_key`` / ``self.lowres_s`` /
    ``self.lowres_noise``.  ``QSample.t`` indexes the diffusion's ``loss_weight`` table, ``QSample.net_t`` (when not None) is the
    time the network reads.  ``ElucidatedDiffusion`` (models/generative/diffusion/edm.py): n ~ randn(B) stands where randint
    stood (``self.t`` holds it), then noise, the label drop and the dropout key, then ``lgm_edm_qsample``.  Everything behind
    q_sample is the plain step."""

    def __init__(self, model, opt, x: torch.Tensor, sync=None, warmup: int = 3, y: Optional[torch.Tensor] = None,
                 accum: Optional[_GradAccumulation] = None):
        from models.generative.diffusion.ddpm import hip_loss_backward_begin, hip_loss_estimate, hip_loss_network
        self.model, self.opt, self.sync, self.accum = model, opt, sync, accum
        self.gd = gd = model.ema.online_model
        self.net = net = gd.model
        self.x = x                                   # static input buffer (copy new batches into it)
        self.one = torch.ones(1, device=x.device)
        net.grad_sync = None                         # collectives are issued by step(), never captured
        fp = net._flat
        self.t = self.noise = self.offset = self.classes = self.dropout_key = self.lowres_s = self.lowres_noise = None
        self.y = net.labels(y, x.shape[0], x.device).clone() if net.num_classes is not None else None
        # (the pipelined variant applies a bucket's Adam slice right behind ITS all-reduce: only with the overlapped exchange)
        # (and a slice cannot be updated before the whole gradient norm exists, or before the last micro-batch)
        self.pipeline = (_STEP_PIPELINE and (sync is None or getattr(sync, "overlap", True))
                         and accum is None and not _clipping(opt))
        self.layout = (LAYOUT_BUCKETS if sync is not None or self.pipeline else LAYOUT_ONE if _ONE_GRAPH else LAYOUT_TWO)
        self_cond = bool(net.self_condition)
        self.pre = self.est = None                   # self-conditioned model only: see the class comment
        # timestep sampler (lgm_hip.tsampler): its draw opens qsample(), its update follows the loss inside hip_loss_network -
        # both inside the capture, its state on the device.  Warm-up and capture run the step: the state is put back after them.
        self.ts = ts = gd.active_t_sampler()
        # progressive distillation (GaussianDiffusion.distill_from): the teacher's grid, table and weights as they are NOW are
        # what the graphs hold - a new round (another teacher, another step count) is a new step object
        self.distill_sig = (gd._distill, gd._distill.table) if gd._distill is not None else None

        def qsample():
            # the diffusion's draws, in the order its forward takes them, and its q_sample launches (the class comment)
            d = gd.draw(self.x, self.y)
            self.t, self.noise, self.offset, self.classes, self.dropout_key = d[:5]
            self.lowres_s, self.lowres_noise = d.lowres or (None, None)
            return gd.qsample(self.x, d, gd.auto_normalize)

        def estimate(q):
            hip_loss_estimate(gd, q.xt, q.t, self.classes, self.dropout_key)

        def begin(q):                                # the saved forward, the loss, its gradient: the backward is open
            loss, ctx = hip_loss_network(gd, q.xt, q.target, q.img, q.t, q.noise, q.offset, True, self.classes,
                                         dropout_key=self.dropout_key, lowres_s=q.lowres_s, net_t=q.net_t)
            fp.zero_grad()
            return loss, hip_loss_backward_begin(ctx, self.one)

        def whole():
            q = qsample()
            if self_cond:
                estimate(q)
            net.backward_run(begin(q)[1])

        # warm-up and capture must not perturb the random stream: a run that captures at batch 0 and a run that
        # resumes from a checkpoint (and captures later) draw the same (t, noise) for the same seed
        rng_state = torch.cuda.get_rng_state(x.device)
        if ts is not None:
            ts.ensure_plan()                         # eager, in front of the snapshot: a replay does not pass through Python
            ts_state = ts.snapshot()
        try:
            _warm_up(whole, warmup)                  # (the WHOLE step: the pieces share workspaces and kernel attributes)
            if self.pipeline:
                net._flush_collect = {}              # the phases hand their reduction rows over instead of launching
            try:
                q, pool = None, None
                if self_cond:
                    self.pre, q, _ = _capture(qsample, 0)
                    pool = self.pre.pool()
                    self.est, _, _ = _capture(lambda: estimate(q), 0, pool)
                    self._q = q                      # keeps the input buffer and the target alive
                self.graphs = []
                for phases in self.layout:
                    def part():
                        if phases[0] == 0:
                            self.loss, self._st = begin(q if self_cond else qsample())
                        net.backward_run(self._st, phases[0], phases[-1])
                    g, _, _ = _capture(part, 0, pool)
                    pool = g.pool() if pool is None else pool        # every later graph: the first one's pool
                    self.graphs.append(g)
                rows = net._flush_collect if self.pipeline else {}
            finally:
                net._flush_collect = None
            buckets = net.bucket_ranges()
            self.ranges = [[r for k in phases for r in buckets[k]] for phases in self.layout]
            if self.pipeline:
                self.reducers = [ops.make_reducer(rows.get(k), x.device) for k in range(4)]
                self.side = torch.cuda.Stream()
                self.events = [torch.cuda.Event() for _ in range(4)]
        finally:
            torch.cuda.set_rng_state(rng_state, x.device)
            if ts is not None:
                ts.restore(ts_state)

    def step(self, batch_idx: int = 0, self_cond: bool = False):
        """``self_cond``: this step's coin (read by a self-conditioned model only)."""
        if self.ts is not None:
            self.ts.ensure_plan()                    # a state loaded since the last step: one eager launch, else a host flag
        if self.pre is not None:                    # draws + q_sample, then the estimate pass when the coin says so
            self.pre.replay()
            if self_cond:
                self.est.replay()
        sync = self.sync
        if self.pipeline:
            self._replay_pipelined()
        elif self.accum is not None:
            self._replay_accumulating()
        else:
            for g, ranges in zip(self.graphs, self.ranges):
                g.replay()
                if sync is not None:
                    for lo, hi in ranges:
                        sync.ready(lo, hi)           # asynchronous, on RCCL's stream, behind the replay just enqueued
            if sync is not None:
                sync.finish()
            self.opt.step()
        self.opt.zero_grad()                         # host flag only: the next backward overwrites
        self.model.on_train_batch_end(None, None, batch_idx)
        return self.loss

    def _replay_accumulating(self):
        """Micro-steps 1 ... K-1: the replays and one accumulate launch.  Micro-step K: ``grad += acc`` per graph over
        that graph's slices, right behind its replay and in front of their ``sync.ready``, so the all-reduces still run
        beside the later graphs; then the tail of a plain step."""
        sync, accum = self.sync, self.accum
        if not accum.stepping:
            for g in self.graphs:
                g.replay()
            accum.stash()
            return
        for g, ranges in zip(self.graphs, self.ranges):
            g.replay()
            if sync is not None:
                for lo, hi in ranges:
                    accum.fold(lo, hi)
                    sync.ready(lo, hi)
        _accumulated_step(self.opt, sync, accum)

    def _replay_pipelined(self):
        sync = self.sync
        fp = self.net._flat
        main, side = torch.cuda.current_stream(), self.side
        inner = getattr(self.opt, "_opt", self.opt)
        group, st = inner.begin_step(fp)
        side.wait_stream(main)                       # whatever touched the weights / gradients before this step
        for k, g in enumerate(self.graphs):
            g.replay()
            self.events[k].record(main)
            with torch.cuda.stream(side):
                side.wait_event(self.events[k])
                ops.launch_reducer(self.reducers[k])             # bucket k's gradients are final after this
                hs = [sync.ready(lo, hi) for lo, hi in self.ranges[k]] if sync is not None else []
                for h in hs:
                    if h is not None:
                        h.wait()                                 # the SIDE stream waits for the exchange, not the host
                for lo, hi in self.ranges[k]:
                    inner.step_slice(fp, group, st, lo, hi)
        main.wait_stream(side)
        if sync is not None:
            sync.finish()
        if hasattr(self.opt, "count_step"):
            self.opt.count_step()                    # MiniTrainer's proxy: one optimizer step


class DDPMFastStep:
    """What ``MiniTrainer.fit`` drives for a ``DDPM`` module (``DDPM.make_fast_step``): the bucketed gradient
    exchange overlapped with the hand-written backward (``FlatGradSync``, N > 1) and the graph replay of
    the step, captured lazily at the first batch.  When capture is not possible (or a batch has another shape)
    the same step runs from eager launches, in the same process, with the same overlapped exchange.
    Logging (``train_loss``) and the reference's periodic in-training sampling (ddpm.py:1017-1027) stay
    outside the graphs."""

    def __init__(self, model, opt, world: int, use_graph: bool = True, accumulate: int = 1):
        from .lightning import FlatGradSync
        self.model, self.opt = model, opt
        self.net = model.ema.online_model.model
        self.sync = FlatGradSync(self.net._flat) if FlatGradSync.wanted(world) else None
        inner = getattr(opt, "_opt", opt)            # MiniTrainer wraps optimizers in a step-counting proxy
        if self.sync is not None:
            inner.grad_scale = self.sync.grad_scale  # 1/N folded into Adam (no divide pass)
        # accumulate_grad_batches: one extra flat buffer and a micro-step count; 1: no buffer, no launch more than before
        self.accum = _GradAccumulation(self.net._flat, accumulate) if int(accumulate) > 1 else None
        self.use_graph = use_graph
        self.graphed: Optional[GraphedDDPMStep] = None
        self.mode = "eager"
        # self-conditioned model: the coin of reference :902, drawn on the host once per step (tests put a sequence here)
        self.coin = lambda: random.random() < 0.5

    def _capture(self, x, y=None):
        try:
            self.graphed = GraphedDDPMStep(self.model, self.opt, x.clone(), self.sync, y=y, accum=self.accum)
            n = len(self.graphed.graphs) + (1 if self.graphed.pre is not None else 0)
            self.mode = ("hipGraph replay (4 graphs/step, weight passes on a side stream)" if self.graphed.pipeline else
                         f"hipGraph replay ({n} graph{'s' if n > 1 else ''}/step)")
            if self.graphed.est is not None:
                self.mode = self.mode[:-1] + ", + the estimate graph on self-conditioned steps)"
        except Exception as e:
            _eager_fallback(self, e)
            self.graphed = None

    def step(self, batch, batch_idx: int = 0):
        from models.generative.diffusion.ddpm import _is_master
        m = self.model
        x = batch[0]
        y = batch[1] if self.net.num_classes is not None else None      # the labels: read by a class-conditional model only
        if getattr(m, "lowres_cond", False):
            m._cond_images = x                       # a super-resolution stage logs samples of the batch at hand
        if m.sample_every and m.global_step % m.sample_every == 0 and _is_master():
            m._log_sample()
        d = m.ema.online_model._distill
        sig = self.graphed.distill_sig if self.graphed is not None else None
        if self.graphed is not None and ((sig is None) != (d is None) or (d is not None and (sig[0] is not d or sig[1] is not d.table))):
            self.graphed = None                      # a new distillation round (or none any more): the graphs held the old one's
        if self.use_graph and self.graphed is None:
            self._capture(x, y)
        self_cond = bool(self.coin()) if self.net.self_condition else False
        if self.graphed is not None and x.shape == self.graphed.x.shape:
            self.graphed.x.copy_(x)
            if y is not None:
                self.graphed.y.copy_(y)
            loss = self.graphed.step(batch_idx, self_cond)
        else:
            accum = self.accum
            # backward phases hand finished buckets to the exchange (an accumulating step exchanges behind its backward:
            # a bucket is final only once the pending sum is added)
            self.net.grad_sync = self.sync if accum is None else None
            gd = m.ema.online_model
            kw = dict(_self_cond=self_cond) if self.net.self_condition else {}
            if y is not None:
                kw["classes"] = y
            loss = gd(x, **kw)
            loss.backward()
            if accum is None:
                if self.sync is not None:
                    self.sync.finish()
                self.opt.step()
            elif accum.stepping:
                self._exchange_accumulated()
                _accumulated_step(self.opt, self.sync, accum)
            else:
                accum.stash()
            self.opt.zero_grad()
            m.on_train_batch_end(None, batch, batch_idx)
            self.net.grad_sync = None
        m.log("train_loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        return loss

    def _exchange_accumulated(self):
        """eager launches / ``flush``: every bucket's pending sum added and handed to the exchange, in bucket order"""
        if self.sync is not None:
            for ranges in self.net.bucket_ranges():
                for lo, hi in ranges:
                    self.accum.fold(lo, hi)
                    self.sync.ready(lo, hi)

    def flush(self):
        """Step on whatever is pending, at the same 1 / K scale (Lightning steps on the last batch of an epoch)."""
        accum = self.accum
        if accum is None or accum.k == 0:
            return
        accum.unstash()
        self._exchange_accumulated()
        _accumulated_step(self.opt, self.sync, accum)
        self.opt.zero_grad()


class ModuleFastStep:
    """Fast step for an automatic-optimisation module whose ``training_step`` is pure device work on one flat
    parameter buffer (VQ-VAE: ~145 launches of 5-15 us, host-bound when issued from Python):
    ``training_step`` + ``backward`` are captured ONCE into a HIP graph at the first batch and replayed; the
    gradient exchange (N > 1: one all-reduce of the flat buffer, 1/N folded into Adam), the fused Adam kernel and
    the module hooks stay eager.  Warm-up and capture must not advance the training state (EMA codebooks, running
    statistics, the random stream): parameters, buffers and the generator state are snapshotted and restored, so
    a run that captures is bit-identical to one that does not.  Falls back to eager launches in the same process
    when capture is not possible, a collective sits inside ``training_step`` (``collective_inside``) or a batch has
    another shape."""

    def __init__(self, model, opt, world: int = 1, use_graph: bool = True, collective_inside: bool = False,
                 accumulate: int = 1):
        self.model, self.opt, self.world = model, opt, world
        self.flat = model._flat
        inner = getattr(opt, "_opt", opt)
        if world > 1:
            inner.grad_scale = 1.0 / world
        self.accum = _GradAccumulation(self.flat, accumulate) if int(accumulate) > 1 else None
        self.use_graph = use_graph and not (collective_inside and world > 1)
        self.captured: Optional[_Captured] = None    # its ``out``: (loss, what training_step logged inside the capture)
        self.static = None                           # the captured step's input tensors
        self._one = None
        self.mode = "eager"

    # ---- one step from eager launches ---------------------------------------------------------------------------
    def _fwd_bwd(self, batch, batch_idx):
        loss = self.model.training_step(batch, batch_idx)
        self.flat.zero_grad()                        # host flag: this backward overwrites the gradient buffer
        one = self._one                              # the backward's seed: made once (autograd would fill a new one per step)
        if one is None or one.device != loss.device or one.dtype != loss.dtype or one.shape != loss.shape:
            one = self._one = torch.ones_like(loss)
        loss.backward(one)
        return loss

    def _optimizer_step(self):
        accum = self.accum
        if accum is not None:
            accum.fold(0, self.flat.total)
            getattr(self.opt, "_opt", self.opt).grad_scale = accum.scale(1.0 / self.world)
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(self.flat.grad)
        self.opt.step()
        if accum is not None:
            accum.stepped()

    def _finish(self, batch, batch_idx):
        if self.accum is None or self.accum.stepping:
            self._optimizer_step()
        else:
            self.accum.stash()
        self.opt.zero_grad()
        self.model.on_train_batch_end(None, batch, batch_idx)

    def flush(self):
        """Step on whatever is pending, at the same 1 / K scale (Lightning steps on the last batch of an epoch)."""
        if self.accum is None or self.accum.k == 0:
            return
        self.accum.unstash()
        self._optimizer_step()
        self.opt.zero_grad()

    def _capture(self, batch):
        m = self.model

        def fn(static):
            # what training_step logs during capture lives in the graph's memory: every replay refreshes those
            # tensors in place, so they are what the module reports after each replayed step
            if hasattr(m, "logged"):
                m.logged.clear()
            return self._fwd_bwd(static, 0), dict(getattr(m, "logged", {}))
        try:
            self.captured = _Captured.of(fn, batch, [m], self.flat.grad.device)
            self.static = self.captured.static
            self.mode = "hipGraph replay (1 graph/step)"
        except Exception as e:
            _eager_fallback(self, e)

    def step(self, batch, batch_idx: int = 0):
        if self.use_graph and self.captured is None:
            self._capture(batch)
        if self.captured is not None and self.captured.matches(batch):
            loss, logs = self.captured.replay(batch)
            if hasattr(self.model, "logged"):
                self.model.logged.update(logs)
        else:
            loss = self._fwd_bwd(batch, batch_idx)
        self._finish(batch, batch_idx)
        return loss


class WGANFastStep:
    """Fast step for the WGAN / WGAN-GP module (manual optimisation, reference wgan.py:58-82): the critic update and
    the generator update are captured ONCE each into a HIP graph — z ~ randn, G forward, (alpha ~ rand, three critic
    forwards, the gradient-penalty double backward | critic forward + input-gradient sweep + G backward) — and
    replayed; the n_critic : 1 schedule (keyed on ``global_step``), the gradient exchange (N > 1: ONE all-reduce of
    the flat buffer the update wrote, 1/N folded into the fused optimizer), the optimizer kernel and logging stay on
    the host.  Warm-up and capture leave the training state (BatchNorm running statistics, random stream) untouched;
    eager fallback in the same process when capture is not possible or a batch has another shape."""

    def __init__(self, model, opts, world: int = 1, use_graph: bool = True):
        from .lightning import FlatGradSync
        self.model, self.world = model, world
        self.d_opt, self.g_opt = opts
        for o in opts:
            inner = getattr(o, "_opt", o)
            if world > 1:
                inner.grad_scale = 1.0 / world
        if world > 1:
            model._grads_prescaled = True
        self.sync = ({"d": FlatGradSync(model.D._flat, beside_backward=False),
                      "g": FlatGradSync(model.G._flat, beside_backward=False)} if world > 1 else None)
        self.use_graph = use_graph
        self.graphs = {}          # "d" / "g" -> _Captured; its ``out``: the update's logs
        self.mode = "eager"

    # the two updates, without exchange / optimizer step (what a graph holds)
    def _critic(self, x):
        m = self.model
        x_hat = m.G.random_sample(x.size(0))
        ld = m._calculate_d_loss(x, x_hat)
        m.D._flat.zero_grad()
        ld["d_loss"].backward()
        return ld

    def _generator(self, x):
        m = self.model
        x_hat = m.G.random_sample(x.size(0))
        ld = m._calculate_g_loss(x_hat)
        m.G._flat.zero_grad()
        ld["g_loss"].backward()
        return ld

    def _capture(self, key, x):
        fn = self._critic if key == "d" else self._generator
        try:
            self.graphs[key] = _Captured.of(lambda static: dict(fn(static[0])), (x,), [self.model], x.device)
            self.mode = "hipGraph replay (critic graph / generator graph)"
        except Exception as e:
            _eager_fallback(self, e)

    def step(self, batch, batch_idx: int = 0):
        m = self.model
        x = batch[0]
        critic = (m.global_step + 1) % (m.hparams.n_critic + 1) != 0
        key = "d" if critic else "g"
        if self.use_graph and key not in self.graphs and m.training:
            self._capture(key, x)
        ent = self.graphs.get(key)
        if ent is not None and ent.matches((x,)):
            logs = ent.replay((x,))
        else:
            logs = self._critic(x) if critic else self._generator(x)
        if self.sync is not None:
            sy = self.sync[key]
            sy.ready(0, sy.flat.total)
            sy.finish()
        opt = self.d_opt if critic else self.g_opt
        opt.step()                                   # the counting proxy advances global_step (the schedule's clock)
        opt.zero_grad()
        m.log_dict(logs, prog_bar=True, logger=True, sync_dist=self.world > 1)
        return logs


class GANFastStep:
    """Fast step for the MLP GAN (manual optimisation, reference gan.py:144-174: one D update, then one G update on the SAME
    ``x_hat``).  What runs in front of the D optimizer step - z ~ randn, G forward with its tape, D on the real and on the
    fake batch, the BCE head, D's backward - and what runs behind it - D forward on that ``x_hat`` with the updated
    weights, the BCE head, the input-gradient sweep through D, G's backward - are captured ONCE into two HIP graphs that
    share one memory pool and one capture stream: the second reads the first's ``x_hat`` and generator tape where the first
    left them.  The gradient exchange (N > 1: ONE all-reduce per update of the flat buffer that update wrote, 1/N folded
    into the fused optimizer), the two optimizer kernels and logging stay on the host.  Warm-up and capture leave
    parameters, running statistics, batch counters and the random stream untouched; eager launches in the same process when
    capture is not possible or a batch has another shape."""

    def __init__(self, model, opts, world: int = 1, use_graph: bool = True):
        from .lightning import FlatGradSync
        self.model, self.world = model, world
        self.d_opt, self.g_opt = opts
        for o in opts:
            if world > 1:
                getattr(o, "_opt", o).grad_scale = 1.0 / world
        if world > 1:
            model._grads_prescaled = True
        self.sync = ({"d": FlatGradSync(model.D._flat, beside_backward=False),
                      "g": FlatGradSync(model.G._flat, beside_backward=False)} if world > 1 else None)
        self.use_graph = use_graph
        self.captured = None      # (_Captured of the D phase: out = (x_hat, logs), _Captured of the G phase: out = logs)
        self.mode = "eager"

    # the two halves of a step, without exchange / optimizer step (what a graph holds)
    def _d_phase(self, x):
        m = self.model
        x_hat = m.G.random_sample(x.size(0))
        ld = m._calculate_d_loss(x, x_hat)
        m.D._flat.zero_grad()
        ld["d_loss"].backward()
        return x_hat, ld

    def _g_phase(self, x_hat):
        m = self.model
        lg = m._calculate_g_loss(x_hat)
        m.G._flat.zero_grad()
        lg["g_loss"].backward()
        return lg

    def _capture(self, x):
        m = self.model
        static = (x.clone(),)
        state = _TrainingState([m], x.device)
        try:
            # the whole step eagerly (the second half consumes the first's tape: the halves cannot warm up apart)
            _warm_up(lambda: self._g_phase(self._d_phase(static[0])[0]), 2)
            ga, out_a, trace_a = _capture(lambda: self._d_phase(static[0]), 0)
            gb, out_b, trace_b = _capture(lambda: self._g_phase(out_a[0]), 0, pool=ga.pool())
            self.captured = (_Captured(ga, static, out_a, trace_a), _Captured(gb, (), out_b, trace_b))
            self.mode = "hipGraph replay (D graph / G graph, one pool)"
        except Exception as e:
            self.captured = None
            _eager_fallback(self, e)
        finally:
            state.restore()

    def _update(self, key, opt):
        if self.sync is not None:
            sy = self.sync[key]
            sy.ready(0, sy.flat.total)
            sy.finish()
        opt.step()
        opt.zero_grad()

    def step(self, batch, batch_idx: int = 0):
        m = self.model
        x = batch[0]
        if self.use_graph and self.captured is None and m.training:
            self._capture(x)
        cap = self.captured
        replay = cap is not None and cap[0].matches((x,))
        x_hat, ld = cap[0].replay((x,)) if replay else self._d_phase(x)
        self._update("d", self.d_opt)
        lg = cap[1].replay(()) if replay else self._g_phase(x_hat)
        self._update("g", self.g_opt)
        logs = {f"train_{k}": v for k, v in {**ld, **lg}.items()}
        m.log_dict(logs, prog_bar=True, logger=True, sync_dist=self.world > 1)
        return logs
