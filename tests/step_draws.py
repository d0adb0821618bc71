"""CPU: what a training step of every diffusion variant draws, in which order, and what it launches - behind the recording
library and the fake graph objects of tests/test_step_trace_host.py (its ``_Session``), so the whole step runs without a
device.

``measure()`` is run twice: by tools/make_golden_step_draws.py on a checkout of the commit BEFORE the draws were folded into
one routine per diffusion, which records tests/golden/step_draws_host.json, and by tests/test_step_draws_host.py on the tree
at hand, which compares.  Nothing here reads how the tree spells its draws: the random functions of torch are wrapped and
every call goes on record (name, shape, sha-256 of what it returned), the operands the network got are read where it gets them
(``Unet.forward_nhwc``), and the step object is read through the attributes it keeps after a replay.

Per kind, under fixed seeds: one eager ``forward`` (with labels where the kind has classes) and its ``backward``; one
``p_losses`` with every explicit operand the kind admits - it must draw nothing; two ``DDPMFastStep.step`` calls (the first
one warms up and captures: its record holds the draws of the three warm-up runs and of the capture; a fake replay runs nothing,
so the second one draws nothing and the step object keeps what the capture drew).  A time the recording library "computed"
(the timestep samplers' ``lgm_tsampler_draw``) is uninitialised memory on the CPU and is left out."""
import contextlib
import hashlib

import pytest
import torch

from test_step_trace_host import KINDS as _TRACE_KINDS
from test_step_trace_host import _Session, _norm

B, SIZE, T = 2, 16, 10
# kind -> (module class, its keywords); the seven of tests/test_step_trace_host.py and the features they leave out
KINDS = {k: ("DDPM", kw) for k, kw in _TRACE_KINDS.items()}
KINDS.update(dropout=("DDPM", dict(dropout=0.1)), lowres=("DDPM", dict(lowres_cond=True, lowres_factor=4)),
             distill=("DDPM", dict(distill_steps=2)), edm=("EDM", dict(learned_sinusoidal_cond=True)),
             edm_classes=("EDM", dict(learned_sinusoidal_cond=True, num_classes=3)))
COINS = (True, False)
STEP_ATTRS = ("t", "noise", "offset", "classes", "dropout_key", "lowres_s", "lowres_noise")


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def sha_trace(calls) -> str:
    """entry points and scalar arguments, pointers left out (``_norm``)"""
    return hashlib.sha256(repr(_norm(calls)).encode()).hexdigest()[:24]


@contextlib.contextmanager
def recorded_draws(log):
    """every call of a random function of torch appends [name, shape, sha] to ``log``"""
    with pytest.MonkeyPatch.context() as mp:
        def wrap(owner, name):
            real = getattr(owner, name)

            def fn(*a, **kw):
                out = real(*a, **kw)
                log.append([name, list(out.shape), sha(out)])
                return out
            mp.setattr(owner, name, fn)
        for name in ("rand", "randn", "randn_like", "randint"):
            wrap(torch, name)
        wrap(torch.Tensor, "random_")
        yield


@contextlib.contextmanager
def network_operands(got):
    """``got``: what the last forward of a ``Unet`` was given - (classes, dropout key, low-resolution levels), hashed"""
    from models.generative.diffusion.ddpm import Unet
    real = Unet.forward_nhwc

    def fwd(self, x, t, save, refresh_weights=True, classes=None, dropout_key=None, drop_pass=0, lowres_s=None, *a, **kw):
        got.update(classes=classes, dropout_key=dropout_key, lowres_s=lowres_s)
        return real(self, x, t, save, refresh_weights, classes, dropout_key, drop_pass, lowres_s, *a, **kw)

    def drop_operands(self, dropout_key, drop_pass):             # ``Unet.drop_operands`` without its is_cuda assertion
        from lgm_hip import ops
        n = len(self.resblocks())
        if dropout_key is None or self.dropout <= 0.0 or not self.training:
            return [None] * n
        return [ops.DropOperands(dropout_key, k, drop_pass, self.drop_thr, self.drop_scale) for k in range(n)]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(Unet, "forward_nhwc", fwd)
        mp.setattr(Unet, "drop_operands", drop_operands)
        yield


def _hashed(d):
    return {k: None if v is None else sha(v) for k, v in d.items()}


def module(kind):
    from models.generative.diffusion import ddpm, edm
    cls, kw = KINDS[kind]
    torch.manual_seed(0)
    if cls == "DDPM":
        m = ddpm.DDPM(img_channels=3, img_size=SIZE, dim=16, diffusion_timesteps=T, ema_update_every=2, **kw)
    else:
        m = edm.EDM(img_channels=3, img_size=SIZE, dim=16, ema_update_every=2, **kw)
    m.sample_every = 0
    m.prepare_hip("cpu")
    m.train()
    g = torch.Generator().manual_seed(1)
    return m, m.configure_optimizers(), (torch.rand(B, 3, SIZE, SIZE, generator=g) * 2 - 1, torch.tensor([0, 2]))


def has_classes(kind) -> bool:
    return KINDS[kind][1].get("num_classes") is not None


def explicit_operands(kind, x):
    """-> (args, kwargs) of a ``p_losses`` call that leaves nothing to draw"""
    cls, kw = KINDS[kind]
    g = torch.Generator().manual_seed(2)
    noise = torch.randn(x.shape, generator=g)
    more = {}
    if has_classes(kind):
        more["classes"] = torch.tensor([1, 3])                   # as the network gets them: 3 is the null label
    if kw.get("dropout"):
        more["_dropout_key"] = torch.tensor([-1234567890123456789])
    if cls == "EDM":
        return (x,), dict(sigma=torch.tensor([0.3, 2.5]), noise=noise, **more)
    if kw.get("offset_noise_strength"):
        more["_offset_noise"] = torch.randn(x.shape[:2], generator=g)
    if kw.get("lowres_cond"):
        more.update(lowres_aug_t=torch.tensor([1, 7]), lowres_noise=torch.randn(x.shape, generator=g))
    if kw.get("self_condition"):
        more["_self_cond"] = True
    t = torch.tensor([9, 4]) if kw.get("distill_steps") else torch.tensor([0, 9])       # (the student's grid: 9, 4, -1)
    return (x, t), dict(noise=noise, **more)


def measure_kind(ses, kind, traces=None):
    """``traces`` (a dict): also filled with every run's launches as ``_norm`` gives them - what a failing test prints"""
    rec = ses.rec
    out = {}

    def run(name, fn, operands):
        draws, start = [], len(rec.calls)
        with recorded_draws(draws):
            fn()
        calls = rec.calls[start:]
        if traces is not None:
            traces[name] = _norm(calls)
        out[name] = {"draws": draws, "operands": _hashed(operands()), "launches": len(calls), "trace": sha_trace(calls)}

    ses.ops.clear_plan_caches()
    m, opt, (x, y) = module(kind)
    gd = m.ema.online_model
    got = {}
    kw = dict(classes=y) if has_classes(kind) else {}
    if KINDS[kind][1].get("self_condition"):
        kw["_self_cond"] = True
    with network_operands(got):
        torch.manual_seed(3)
        run("forward", lambda: gd(x, **kw).backward(), lambda: dict(got))
        got.clear()
        args, kw = explicit_operands(kind, x)
        torch.manual_seed(4)
        run("p_losses", lambda: gd.p_losses(*args, _normalize=True, **kw), lambda: dict(got))
        out.update(steps(ses, kind, run))
    return out


def steps(ses, kind, run):
    ses.ops.clear_plan_caches()
    m, opt, batch = module(kind)
    fast = ses.graph.DDPMFastStep(m, opt, 1, use_graph=True)
    coins = iter(COINS)
    fast.coin = lambda: next(coins)
    torch.manual_seed(5)
    timed = bool(KINDS[kind][1].get("t_sampler"))                # t comes out of a launch: not there on the CPU

    def step_operands():
        gs = fast.graphed
        return {a: None if a == "t" and timed else getattr(gs, a) for a in STEP_ATTRS}
    for i in range(len(COINS)):
        run(f"step{i}", lambda: fast.step(batch, i), step_operands)
    return {"mode": fast.mode}


def measure(kinds=None, traces=None):
    out = {}
    for kind in (KINDS if kinds is None else kinds):
        with pytest.MonkeyPatch.context() as mp:
            state = torch.get_rng_state()
            try:
                out[kind] = measure_kind(_Session(mp), kind, traces)
            finally:
                torch.set_rng_state(state)
    return out
