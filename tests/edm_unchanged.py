"""What the sinusoidal (discrete-time) paths compute and launch, as bits and as a launch trace: one eager DDPM training step,
two graph-replayed ones and a DDIM chain (eager and graph-replayed) of a small network under fixed seeds.

``measure(dev)`` is run twice: by tools/make_golden_edm_unchanged.py on a checkout of the commit BEFORE the Fourier embedding
and elucidated diffusion were added, which records tests/golden/diffusion_edm_unchanged.json, and by tests/test_hip_edm.py on
the tree at hand, which compares.  The trace is the order of C-ABI entry points that pass through ``ops.lib()`` - the proxy
idea of the recorders in tests/test_step_trace_host.py and tests/test_sampler_trace_host.py, here in front of the real
library.  Every traced run is preceded by the same run on a twin model, so the process-wide plan caches are warm whether or
not other tests ran before; what is per model (flat storage, Winograd operand registration) is fresh in both."""
import hashlib
import os
import struct

import torch


class _Tracing:
    """the real library with every ``lgm_*`` call's name appended to ``calls``"""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("lgm_") or not callable(f):
            return f

        def call(*a):
            self._calls.append(name)
            return f(*a)
        return call


class traced:
    def __enter__(self):
        from lgm_hip import ops
        self.ops, self.saved, self.calls = ops, ops.lib, []
        proxy = _Tracing(ops.lib(), self.calls)
        ops.lib = lambda: proxy
        return self.calls

    def __exit__(self, *exc):
        self.ops.lib = self.saved


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def bits(v) -> str:
    return struct.pack(">f", float(v)).hex()


def _module(dev):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(21)
    m = DDPM(img_size=16, dim=16, lr=1e-3, ema_update_every=1, sampling_timesteps=5)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m, m.configure_optimizers()


def measure(dev):
    g = torch.Generator().manual_seed(22)
    xs = [torch.rand(4, 3, 16, 16, generator=g).to(dev) for _ in range(2)]
    out = {}

    def eager_step(m, opt):
        torch.manual_seed(5)
        loss = m.ema.online_model(xs[0])
        loss.backward()
        opt.step()
        opt.zero_grad()
        m.on_train_batch_end(None, None, 0)
        torch.cuda.synchronize()
        return loss

    eager_step(*_module(dev))                                            # warms the process-wide plan caches
    m, opt = _module(dev)
    with traced() as calls:
        loss = eager_step(m, opt)
    net = m.ema.online_model.model
    out["step"] = {"trace": list(calls), "loss": bits(loss.detach()), "grad": sha(net._flat.grad), "params": sha(net._flat.data),
                   "ema": sha(m.ema.ema_model.model._flat.data)}

    m, opt = _module(dev)
    fast = m.make_fast_step(opt, 1, True)
    torch.manual_seed(5)
    losses = [bits(fast.step((x.clone(), None), i).detach().reshape(())) for i, x in enumerate(xs)]
    torch.cuda.synchronize()
    out["graph_steps"] = {"mode": fast.mode, "losses": losses, "params": sha(m.ema.online_model.model._flat.data),
                          "ema": sha(m.ema.ema_model.model._flat.data), "t": fast.graphed.t.tolist()}

    gd = m.ema.ema_model
    gd.eval()

    def chain():
        torch.manual_seed(6)
        img = gd.sample(batch_size=2)
        torch.cuda.synchronize()
        return img

    replayed = chain()
    old = os.environ.get("LGM_NO_SAMPLER_GRAPH")
    os.environ["LGM_NO_SAMPLER_GRAPH"] = "1"
    try:
        chain()
        with traced() as calls:
            eager = chain()
    finally:
        if old is None:
            del os.environ["LGM_NO_SAMPLER_GRAPH"]
        else:
            os.environ["LGM_NO_SAMPLER_GRAPH"] = old
    out["ddim"] = {"trace": list(calls), "image": sha(eager), "image_graph_replay": sha(replayed), "mean": bits(eager.mean())}
    return out
