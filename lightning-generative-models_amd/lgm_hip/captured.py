"""What the graph-replayed inference steps share: ``sampler._GraphedChain`` and ``likelihood._GraphedVLB`` are ``_CapturedStep``s
kept per network by ``_cached_step``.  ``_warm_up`` also serves the training steps of ``graph.py``."""
from __future__ import annotations

import os
import sys
import weakref

import torch

# net -> {key: captured step, or the countdown of a failed capture}.  Weak on the network: a model that goes away takes its
# graphs (and their memory pool) with it.  Every entry remembers which flat parameter storage its launches were captured
# against (``_CapturedStep.matches``): a graph bakes buffer ADDRESSES in, so after prepare_hip() rebuilt the flat storage
# (model.to(), replaced parameter storage) the entry is dropped and the step recaptured.
_GRAPHS = weakref.WeakKeyDictionary()
_CAPTURE_RETRY_AFTER = 8      # a failed capture is retried after this many eager chains, not cached for ever


def _warm_up(fn, n: int):
    """``n`` eager runs of ``fn`` on a side stream (they size workspaces and set kernel attributes), joined before return."""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(n):
            fn()
    cur.wait_stream(side)
    torch.cuda.synchronize()


def _segments(n: int, max_steps: int):
    """[(lo, hi)]: the steps of a chain of n in table-sized pieces, in order; a chain is never truncated to its tables"""
    if max_steps < 1:
        raise ValueError(f"max_steps must be at least 1, got {max_steps}")
    return [(lo, min(lo + max_steps, n)) for lo in range(0, n, max_steps)]


class _CapturedStep:
    """One step captured against a network's flat storage and replayed once per step of a run.  The step reads its time from
    ``ttable[counter]`` and its row of ``row`` floats from ``table[counter]`` and advances the counter.  A subclass allocates
    its other static buffers, hands ``_capture`` its ``one_step`` closure and drives ``_replay`` from its ``run``."""

    def __init__(self, net, dev, max_steps: int, row: int):
        self._net = weakref.ref(net)                 # the cache is keyed weakly on the network: no strong reference here
        fp = net._flat
        # identity of everything whose address the captured launches carry: the flat object and its buffers
        self._bound = (weakref.ref(fp), fp.data.data_ptr(),
                       None if fp.data_uf is None else fp.data_uf.data_ptr(),
                       None if fp.data_t is None else fp.data_t.data_ptr())
        self.max_steps = max_steps
        self.table = torch.zeros((max_steps, row), device=dev)
        self.ttable = torch.zeros(max_steps, dtype=torch.long, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.inject = False                          # read by ``one_step``: noise from the static buffers, not drawn

    def matches(self, net) -> bool:
        """True while the network still owns the flat storage this step was captured against."""
        fp = net._flat
        ref, data, uf, dt = self._bound
        return (fp is not None and ref() is fp and fp.still_bound() and fp.data.data_ptr() == data
                and (None if fp.data_uf is None else fp.data_uf.data_ptr()) == uf
                and (None if fp.data_t is None else fp.data_t.data_ptr()) == dt)

    def _capture(self, one_step, variants, dev):
        """``self.graphs[inject]`` for every ``inject`` of ``variants``: two eager warm-up runs, then one capture each.  It
        leaves the random stream where it was."""
        self._net().refresh_derived_weights(False)
        rng_state = torch.cuda.get_rng_state(dev)
        _warm_up(one_step, 2)
        self.graphs = {}
        for inject in variants:
            self.inject = inject
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                one_step()
            self.graphs[inject] = g
        torch.cuda.set_rng_state(rng_state, dev)

    def _replay(self, times, rows, inject: bool, refill=None, before=None, after=None):
        """times[i], rows[i] per step.  A run longer than the tables goes in table-sized segments: refill the tables
        (``refill(lo, hi)``: a subclass's further ones), zero the counter, replay once per step (``before(i)`` copies what step i
        injects), then ``after(lo, hi)`` copies out what the segment wrote."""
        graph = self.graphs[inject]
        for lo, hi in _segments(len(times), self.max_steps):
            self.table[:hi - lo].copy_(torch.tensor(rows[lo:hi], dtype=torch.float32))
            self.ttable[:hi - lo].copy_(torch.tensor(times[lo:hi], dtype=torch.long))
            if refill is not None:
                refill(lo, hi)
            self.counter.zero_()
            for i in range(lo, hi):
                if before is not None:
                    before(i)
                graph.replay()
            if after is not None:
                after(lo, hi)


def _cached_step(net, key, build, what: str, dev):
    """-> the network's captured step under ``key``, built by ``build()`` on first use and again once the entry no longer
    ``matches`` the network, or None: graph replay is disabled (``LGM_NO_SAMPLER_GRAPH=1``) or ``dev`` is no GPU - nothing is
    looked up or built then -, or ``build`` raised (one line on stderr, ``what`` in it) now or at one of the last
    ``_CAPTURE_RETRY_AFTER`` calls for this key.  The caller then goes on with eager launches."""
    if os.environ.get("LGM_NO_SAMPLER_GRAPH", "0") == "1" or dev.type != "cuda":
        return None
    per_net = _GRAPHS.setdefault(net, {})
    ent = per_net.get(key)
    if isinstance(ent, int):                         # a capture failed earlier: eager for a while, then try again
        if ent > 0:
            per_net[key] = ent - 1
            return None
        ent = None
    elif ent is not None and not ent.matches(net):
        ent = None                                   # captured against buffers the network no longer uses
    if ent is None:
        try:
            ent = build()
        except Exception as e:  # capture is an optimisation
            print(f"[lgm_hip] {what} graph capture unavailable ({type(e).__name__}: {e}); eager launches",
                  file=sys.stderr, flush=True)
            per_net[key] = _CAPTURE_RETRY_AFTER
            return None
        per_net[key] = ent
    return ent
