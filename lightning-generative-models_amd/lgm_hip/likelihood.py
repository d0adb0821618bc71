"""The variational bound of a trained diffusion in bits per dimension, on the HIP engine.

Ho et al. 2020 (eq. 5, the table's NLL column) and Nichol & Dhariwal 2021 (``calc_bpd_loop``); an extension of the reference,
which has no likelihood evaluation.  For held-out images x0 the bound is
    L = L_prior + sum_{t >= 1} KL(q(x_{t-1} | x_t, x0) || p(x_{t-1} | x_t)) - log p(x0 | x_1)
every term a mean over a sample's elements, divided by ln 2.  Per evaluated timestep t: x_t = q_sample(x0, t, noise), ONE
network forward, and one reducing launch (``vlb_term_kernel``) that writes the term, mean (x0_pred - x0)^2 and mean (eps_pred -
noise)^2 of every sample.  T forwards: a hot path of the shape of sampling, replayed as a captured graph like it.

Top down:
  * ``vlb_plan``: one row of ``VLB_ROW`` float32 scalars per evaluated timestep and a last row for the prior, every scalar
    computed in float64 and rounded once.  Host arithmetic on ``math`` only: no device, no library.
  * ``_eager_terms``: the loop in eager launches; ``_GraphedVLB``: one captured step per ``_vlb_key`` - t[b] <- time
    table[counter], the noise draw, q_sample into the static input buffer, forward, the reducer from row table[counter] into
    output row counter, counter += 1 - replayed once per timestep with no Python between the launches, no host sync and no
    allocation.  It lives in ``sampler._GRAPHS`` beside the sampling steps of its network under a key no sampler can have.
  * ``vlb_terms``: the public function behind ``GaussianDiffusion.vlb_terms``; the prior row is one more eager launch, and the
    host reads the [n + 1, 3, B] result once, the only synchronisation.

``variance="learned"`` (a ``Unet(learned_variance=True)``): every element's log-variance is interpolated between log beta_t and
log beta~_t by the network's variance lane (``learned_table``; the device function the hybrid training loss uses).  Otherwise
the model's variance is fixed, by Nichol & Dhariwal's two conventions:
``fixed_small`` = the posterior variance beta~_t, ``fixed_large`` = beta_t, both with t = 0 taking log beta~_1 - not the
reference's ``posterior_log_variance_clipped[0]`` = log 1e-20, under which the decoder would be a step function.
"""
from __future__ import annotations

import math
import struct
from collections import namedtuple
from typing import List, Optional

import torch

from . import ops, sampler
from .captured import _CapturedStep, _cached_step
from .flat import _r4

VLB_ROW = 12                                   # floats per row; the kernel reads the first ten, all twelve of a learned kind
KL, DECODER, PRIOR = 0, 1, 2                   # row[6]
KL_LEARNED, DECODER_LEARNED = 3, 4             # row[6] of a learned-variance network's rows (variance="learned")
VARIANCES = ("fixed_small", "fixed_large")     # the fixed conventions; "learned" is accepted beside them
VLBTerms = namedtuple("VLBTerms", "total_bpd prior_bpd vb xstart_mse mse timesteps")


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _tables64(gd):
    """(betas, alphas_cumprod, posterior_log_variance_clipped) as lists of Python floats: the diffusion's own tables (built in
    float64, kept in float32 - the values its samplers use), widened"""
    return tuple([float(v) for v in getattr(gd, n).detach().double().cpu().tolist()]
                 for n in ("betas", "alphas_cumprod", "posterior_log_variance_clipped"))


def learned_table(gd):
    """-> T rows of 8 float32 values (log beta_t, log beta~_t, lv_q, P1, P2, 0, 0, 0): the per-t scalars of a learned-variance
    diffusion, shared by the hybrid loss (``GaussianDiffusion.learned_table``), the ancestral step and the learned rows of
    ``vlb_plan``.  log beta~_t = ``posterior_log_variance_clipped[t]`` for t >= 1 and log beta~_1 at t = 0 (this module's
    convention, not the reference's log 1e-20); lv_q = ``posterior_log_variance_clipped[t]``; P1 / P2 =
    ``posterior_mean_coef1/2[t]``.  The model's log-variance of an element is f log beta_t + (1 - f) log beta~_t with f = (v +
    1) / 2, v the network's variance lane.  float64 from the diffusion's own tables, rounded once.  Pure Python."""
    betas, _, lv_q = _tables64(gd)
    T = len(betas)
    p1, p2 = ([float(v) for v in getattr(gd, n).detach().double().cpu().tolist()]
              for n in ("posterior_mean_coef1", "posterior_mean_coef2"))
    first = lv_q[1] if T > 1 else math.log(betas[0])
    return [(_f32(math.log(betas[t])), _f32(lv_q[t] if t else first), _f32(lv_q[t]), _f32(p1[t]), _f32(p2[t]), 0.0, 0.0, 0.0)
            for t in range(T)]


def vlb_plan(gd, timesteps=None, variance: str = "fixed_small"):
    """-> n + 1 rows of ``VLB_ROW`` float32 values: one per timestep of ``timesteps`` (default T - 1 ... 0; else distinct ints
    in [0, T), evaluated in the order given), then the prior's.  A row is
        (A, S, R, Rm1, P1, P2, kind, KC, KW, inv_std, lv_p, lv_q)
    (A, S, R, Rm1) the head ``predictions_one`` reads (the diffusion's own float32 tables at t), P1 / P2 =
    ``posterior_mean_coef1/2[t]``, kind ``KL`` (t >= 1), ``DECODER`` (t = 0) or ``PRIOR``.  With lv_q =
    ``posterior_log_variance_clipped[t]`` (log max(beta~_t, 1e-20), the reference's clipping) and the model's log-variance
    lv_p (``fixed_small``: log beta~_t, ``fixed_large``: log beta_t, both log beta~_1 at t = 0):
        KL       KC = 0.5 (-1 + lv_p - lv_q + exp(lv_q - lv_p)), KW = 0.5 exp(-lv_p): the KL per element in nats is KC + KW d^2,
                 d the difference of the posterior means.  ``fixed_small``: KC == 0.0 exactly.
        DECODER  inv_std = exp(-0.5 lv_p)
        PRIOR    slots 10 / 11 hold acp_{T-1} and log(1 - acp_{T-1}); KC = 0.5 (-1 - log(1 - acp) + (1 - acp)) and KW = 0.5 acp,
                 so that the KL per element is KC + KW x0^2 (the sum in KC cancels to about acp^2 / 2: float64 here, not float32
                 on the device).
    ``variance="learned"`` (a learned-variance network only): kind ``KL_LEARNED`` / ``DECODER_LEARNED``, slots 7 - 9 zero and
    slots 10 / 11 = (log beta_t, log beta~_t) of ``learned_table``; the kernel forms every element's own log-variance from them
    and the network's variance lane.  The prior row is the same.
    Everything in float64 from the diffusion's tables, rounded once.  Pure Python: no device, no library."""
    learned = variance == "learned"
    if learned and not getattr(gd.model, "learned_variance", False):
        raise ValueError("variance='learned' needs a model built with learned_variance=True")
    if variance not in VARIANCES and not learned:
        raise ValueError(f"variance must be one of {VARIANCES + ('learned',)}, got {variance!r}")
    T = int(gd.num_timesteps)
    ts = list(reversed(range(T))) if timesteps is None else [int(t) for t in timesteps]
    if any(not 0 <= t < T for t in ts):
        raise ValueError(f"timesteps must lie in [0, {T}), got {[t for t in ts if not 0 <= t < T]}")
    if len(set(ts)) != len(ts):
        raise ValueError("timesteps must be distinct")
    betas, acp, lv_q = _tables64(gd)
    first = lv_q[1] if T > 1 else math.log(betas[0])
    lv_p = [first] + ([lv_q[t] for t in range(1, T)] if variance == "fixed_small" else [math.log(b) for b in betas[1:]])
    hs = sampler._host_schedule(gd)
    lt = learned_table(gd) if learned else None
    rows = []
    for t in ts:
        A, Bv, R, Rm1 = sampler._head(hs, t)
        head = (A, -Bv, R, Rm1, float(hs["posterior_mean_coef1"][t]), float(hs["posterior_mean_coef2"][t]))
        if learned:
            rows.append(head + (float(KL_LEARNED if t else DECODER_LEARNED), 0.0, 0.0, 0.0, lt[t][0], lt[t][1]))
        elif t == 0:
            rows.append(head + (float(DECODER), 0.0, 0.0, _f32(math.exp(-0.5 * lv_p[0])), _f32(lv_p[0]), _f32(lv_q[0])))
        else:
            d = lv_q[t] - lv_p[t]
            kc = 0.5 * (math.expm1(d) - d)                     # -1 - d + e^d without the cancellation at small d
            rows.append(head + (float(KL), _f32(kc), _f32(0.5 * math.exp(-lv_p[t])), 0.0, _f32(lv_p[t]), _f32(lv_q[t])))
    a, l1m = acp[-1], math.log1p(-acp[-1])
    rows.append((0.0,) * 6 + (float(PRIOR), _f32(0.5 * (-1.0 - l1m + (1.0 - a))), _f32(0.5 * a), 0.0, _f32(a), _f32(l1m)))
    return rows


def _byval(row):
    """a row as ``lgm_vlb_term`` takes it: ten scalars, the kind an int"""
    return (*row[:6], int(row[6]), *row[7:10])


def _qsample(gd, img, nz, t, sa, sb, xin):
    """x_t into the x slice of the input buffer (zeros into a self-conditioning slice and the padding); no target wanted"""
    net = gd.model
    B, C, H, W = img.shape
    ops.lib().lgm_qsample_target_slice(img.data_ptr(), nz.data_ptr(), None, 0.0, t.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                       1 if gd.auto_normalize else 0, sampler._objective(gd), xin.data_ptr(), net.in_pitch,
                                       net.x_off, net.sc_off, None, _r4(C), B, C, H * W, _r4(C), ops.stream())


def _launch_term(gd, img, nz, xin, v, clip: bool, out, *, row=None, at: int = 0, table=None, counter=None):
    """The reducer of one timestep: the row by value into output row ``at``, or row ``table[counter]`` into output row
    ``counter`` (the captured step, which also advances the counter).  A prior row takes ``nz = xin = v = None``."""
    net = gd.model
    B, C, H, W = img.shape
    src = (img.data_ptr(), ops._p(nz), 1 if gd.auto_normalize else 0, ops._p(xin), net.in_pitch, net.x_off, ops._p(v),
           _r4(C) if v is None else ops.pitch(v), B, C, H * W, sampler._objective(gd), 1 if clip else 0)
    if getattr(net, "learned_variance", False) and v is not None:
        # a network with the variance head: one entry point for both forms and every kind (the kernel reads the kind from the
        # row; a fixed-variance row is evaluated as ever, from the prediction lanes alone)
        if table is not None:
            ops.lib().lgm_vlb_term_learned(*src, *((0.0,) * 6), 0, 0.0, 0.0, table.data_ptr(), VLB_ROW, counter.data_ptr(),
                                           out.data_ptr(), out.shape[0], 0, 1, ops.stream())
        elif int(row[6]) in (KL_LEARNED, DECODER_LEARNED):
            ops.lib().lgm_vlb_term_learned(*src, *row[:6], int(row[6]), row[10], row[11], None, 0, None, out.data_ptr(),
                                           out.shape[0], at, 0, ops.stream())
        else:
            ops.lib().lgm_vlb_term(*src, *_byval(row), out.data_ptr(), out.shape[0], at, ops.stream())
    elif table is not None:
        ops.lib().lgm_vlb_term_table(*src, table.data_ptr(), VLB_ROW, counter.data_ptr(), out.data_ptr(), out.shape[0], 1,
                                     ops.stream())
    else:
        ops.lib().lgm_vlb_term(*src, *_byval(row), out.data_ptr(), out.shape[0], at, ops.stream())


def _eager_terms(gd, img, times, rows, noises, classes, clip: bool):
    """the n timesteps in eager launches -> [n, 3, B] on the device"""
    net = gd.model
    B, C, H, W = img.shape
    dev = img.device
    out = torch.zeros((len(times), 3, B), device=dev)
    xin = torch.zeros((B, H, W, net.in_pitch), device=dev)
    for i, (t, row) in enumerate(zip(times, rows)):
        tb = torch.full((B,), t, device=dev, dtype=torch.long)
        nz = noises[i] if noises is not None else torch.randn(img.shape, device=dev)
        _qsample(gd, img, nz, tb, gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod, xin)
        v = net.forward_guided(xin, tb, classes, 1.0)
        _launch_term(gd, img, nz, xin, v, clip, out, row=row, at=i)
    return out


class _GraphedVLB(_CapturedStep):
    """A ``_CapturedStep`` of one evaluation step for a (network, batch shape, objective, clip), its rows ``VLB_ROW`` wide.  It
    adds the static image, noise and input buffer, the schedule's two q_sample tables and the [max_steps, 3, B] output, whose
    rows ``run`` copies out behind every segment."""

    def __init__(self, gd, shape, clip: bool, max_steps: int = 4096):
        net = gd.model
        B, C, H, W = shape
        dev = gd.betas.device
        super().__init__(net, dev, max_steps, VLB_ROW)
        self.shape = shape
        self.img = torch.zeros(shape, device=dev)
        self.noise = torch.zeros(shape, device=dev)                   # injected noise goes here
        self.x = torch.zeros((B, H, W, net.in_pitch), device=dev)
        self.t = torch.zeros(B, dtype=torch.long, device=dev)
        self.sa = torch.zeros(gd.num_timesteps, device=dev)           # a diffusion's tables are copied in per run: two
        self.sb = torch.zeros(gd.num_timesteps, device=dev)           # diffusions of one length may share the step
        self.out = torch.zeros((max_steps, 3, B), device=dev)
        self.classes = net.labels(None, B, dev).clone() if net.num_classes is not None else None

        def one_step():
            ops.lib().lgm_sampler_time(self.ttable.data_ptr(), self.counter.data_ptr(), self.t.data_ptr(), B, ops.stream())
            nz = self.noise if self.inject else torch.randn(shape, device=dev)
            _qsample(gd, self.img, nz, self.t, self.sa, self.sb, self.x)
            v = net.forward_guided(self.x, self.t, self.classes, 1.0, refresh_weights=False)
            _launch_term(gd, self.img, nz, self.x, v, clip, self.out, table=self.table, counter=self.counter)

        self._capture(one_step, (False, True), dev)

    def run(self, gd, img, times, rows, noises, classes=None):
        """times[i], rows[i] (``VLB_ROW`` floats) per timestep; noises: None (draw on the device) or one NCHW tensor per
        timestep.  -> [n, 3, B] on the device.  More timesteps than table rows are replayed in table-sized segments."""
        if self.classes is not None:
            self.classes.copy_(classes)
        self._net().refresh_derived_weights(False)   # the weights may have moved since the last evaluation (EMA updates)
        self.img.copy_(img)
        self.sa.copy_(gd.sqrt_alphas_cumprod)
        self.sb.copy_(gd.sqrt_one_minus_alphas_cumprod)
        res = torch.empty((len(times), 3, self.shape[0]), device=img.device)
        inject = noises is not None
        self._replay(times, rows, inject, before=(lambda i: self.noise.copy_(noises[i])) if inject else None,
                     after=lambda lo, hi: res[lo:hi].copy_(self.out[:hi - lo]))
        return res


def _vlb_key(gd, shape, clip: bool):
    """The cache key of a captured evaluation step under its network.  It starts with "vlb": a sampler's key (``_graph_key``)
    starts with a shape tuple, "dpm++", "dynthresh" or "inpaint".  The variance choice lives in the table, not here."""
    return ("vlb", gd.objective, bool(clip), tuple(shape), bool(gd.auto_normalize), int(gd.num_timesteps))


def _graph_vlb(gd, shape, clip: bool) -> Optional[_GraphedVLB]:
    """-> the network's ``_GraphedVLB`` under ``_vlb_key`` from ``_cached_step``, or None (graph replay disabled, no device,
    capture failed: eager launches)"""
    net = gd.model
    net.prepare_hip(gd.betas.device)
    return _cached_step(net, _vlb_key(gd, shape, clip), lambda: _GraphedVLB(gd, tuple(shape), clip), "likelihood",
                        gd.betas.device)


@torch.no_grad()
def vlb_terms(gd, img, *, timesteps=None, noise: Optional[List[torch.Tensor]] = None, clip_denoised: bool = True,
              variance: str = "fixed_small", classes=None) -> VLBTerms:
    """See ``GaussianDiffusion.vlb_terms``.  The result's tensors are float64 on the host: the device's float32 values, read
    once, and ``total_bpd`` their sum over the rows in row order."""
    net = gd.model
    if img.dim() != 4 or tuple(img.shape[1:]) != (gd.channels, gd.img_size, gd.img_size):
        raise ValueError(f"img must be [B, {gd.channels}, {gd.img_size}, {gd.img_size}], got {tuple(img.shape)}")
    rows = vlb_plan(gd, timesteps, variance)
    times = list(reversed(range(gd.num_timesteps))) if timesteps is None else [int(t) for t in timesteps]
    shape = tuple(img.shape)
    dev = gd.betas.device
    if noise is not None:
        noise = list(noise)
        if len(noise) != len(times) or any(tuple(z.shape) != shape for z in noise):
            raise ValueError(f"noise must be {len(times)} tensors of shape {shape}, one per evaluated timestep")
        noise = [z.to(dev).float().contiguous() for z in noise]
    net.prepare_hip(dev)
    classes = net.labels(classes, shape[0], dev)
    img = img.to(dev).float().contiguous()
    clip = bool(clip_denoised)
    n = len(times)
    gv = _graph_vlb(gd, shape, clip) if n else None
    if gv is not None:
        terms = gv.run(gd, img, times, rows[:n], noise, classes)
    else:
        terms = _eager_terms(gd, img, times, rows[:n], noise, classes, clip)
    prior = torch.zeros((1, 3, shape[0]), device=dev)
    _launch_term(gd, img, None, None, None, clip, prior, row=rows[n], at=0)
    host = torch.cat([terms, prior]).double().cpu()            # the one read: [n + 1, 3, B]
    vb, prior_bpd = host[:n, 0], host[n, 0]
    total = None
    if n == gd.num_timesteps:
        total = torch.zeros_like(prior_bpd)
        for i in range(n):                                     # float64, in row order, the prior last
            total += vb[i]
        total += prior_bpd
    return VLBTerms(total, prior_bpd, vb, host[:n, 1], host[:n, 2], tuple(times))
