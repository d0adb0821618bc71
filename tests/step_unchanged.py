"""What a training step of every diffusion variant computes, draws and launches on the device, as bits: per kind one eager
step (forward, backward, Adam, EMA) and two graph-replayed ones of a small network under fixed seeds.

``measure(dev)`` is run by tools/make_golden_step_unchanged.py on a checkout of the commit BEFORE the draws were folded into
one routine per diffusion - twice, a kind is written only where both runs agree -, which records
tests/golden/diffusion_step_unchanged.json, and by tests/test_hip_step_unchanged.py on the tree at hand, which compares.  The
kinds are those of tests/step_draws.py; tests/edm_unchanged.py (whose tracing proxy and twin warm-up this follows) pins the
plain step's trace by name and stays as it is."""
import hashlib

import torch

from edm_unchanged import bits, sha, traced
from step_draws import COINS, KINDS, STEP_ATTRS, has_classes

B, SIZE, T = 4, 16, 10


def module(kind, dev):
    from models.generative.diffusion import ddpm, edm
    cls, kw = KINDS[kind]
    torch.manual_seed(21)
    if cls == "DDPM":
        m = ddpm.DDPM(img_size=SIZE, dim=16, lr=1e-3, ema_update_every=1, diffusion_timesteps=T, **kw)
    else:
        m = edm.EDM(img_size=SIZE, dim=16, lr=1e-3, ema_update_every=1, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m, m.configure_optimizers()


def measure_kind(kind, dev):
    g = torch.Generator().manual_seed(22)
    xs = [torch.rand(B, 3, SIZE, SIZE, generator=g).to(dev) for _ in range(2)]
    y = (torch.arange(B) % 3).to(dev) if has_classes(kind) else None
    kw = dict(classes=y) if y is not None else {}
    if KINDS[kind][1].get("self_condition"):
        kw["_self_cond"] = COINS[0]

    def eager_step(m, opt):
        torch.manual_seed(5)
        loss = m.ema.online_model(xs[0], **kw)
        loss.backward()
        opt.step()
        opt.zero_grad()
        m.on_train_batch_end(None, None, 0)
        torch.cuda.synchronize()
        return loss

    eager_step(*module(kind, dev))                                       # warms the process-wide plan caches
    m, opt = module(kind, dev)
    with traced() as calls:
        loss = eager_step(m, opt)
    net = m.ema.online_model.model
    out = {"eager": {"launches": len(calls), "trace": hashlib.sha256("\n".join(calls).encode()).hexdigest()[:24],
                     "loss": bits(loss.detach()), "grad": sha(net._flat.grad), "params": sha(net._flat.data),
                     "ema": sha(m.ema.ema_model.model._flat.data)}}

    m, opt = module(kind, dev)
    fast = m.make_fast_step(opt, 1, True)
    coins = iter(COINS)
    fast.coin = lambda: next(coins)
    torch.manual_seed(5)
    steps = []
    for i, x in enumerate(xs):
        loss = bits(fast.step((x.clone(), y), i).detach().reshape(()))
        torch.cuda.synchronize()
        gs = fast.graphed
        steps.append({"loss": loss, **{a: None if getattr(gs, a, None) is None else sha(getattr(gs, a)) for a in STEP_ATTRS}})
    out["graph"] = {"mode": fast.mode, "steps": steps, "params": sha(m.ema.online_model.model._flat.data),
                    "ema": sha(m.ema.ema_model.model._flat.data)}
    return out


def measure(dev, kinds=None):
    return {kind: measure_kind(kind, dev) for kind in (KINDS if kinds is None else kinds)}


def flatten(d, prefix=""):
    """{"a": {"b": 1}} -> {"a.b": 1}; a list's entries under their index"""
    if isinstance(d, list):
        d = {str(i): v for i, v in enumerate(d)}
    if not isinstance(d, dict):
        return {prefix[:-1]: d}
    out = {}
    for k, v in d.items():
        out.update(flatten(v, f"{prefix}{k}."))
    return out
