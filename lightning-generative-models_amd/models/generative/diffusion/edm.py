"""Elucidated diffusion (Karras et al. 2022, "Elucidating the Design Space of Diffusion-Based Generative Models"; an extension
of the reference - the library its ``ddpm.py`` was taken from ships it as ``ElucidatedDiffusion`` around the same ``Unet``) on
the MI355X HIP engine: a continuous noise level sigma, the preconditioned denoiser, the log-normal sigma draw in training and
the rho-schedule with the second-order Heun sampler.

The network is a ``Unet(learned_sinusoidal_cond=True | random_fourier_features=True)``: it reads c_noise = ln(sigma) / 4 as a
real-valued time.  Definitions, host planning and the row layout: ``lgm_hip/edm.py``; the elementwise launches around the
network's forwards: ``csrc/edm.hip``.  Training runs on the machinery of the DDPM step (``lgm_hip.graph``) - the saved forward,
the weighted MSE over a one-entry weight table, the four backward phases, Adam and the EMA are untouched; only the draws and
the q_sample launch differ (``ElucidatedDiffusion.draw`` / ``.qsample``: the protocol of ``ddpm.Diffusion``)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from lgm_hip import edm as plan
from lgm_hip import ops
from lgm_hip.captured import _CapturedStep, _cached_step
from lgm_hip.flat import _r4

from .ddpm import Diffusion, DiffusionModule, QSample, StepDraws, Unet, hip_loss_network


class ElucidatedDiffusion(Diffusion):
    """``ElucidatedDiffusion(model, img_size=...)`` around a fourier ``Unet`` (anything else is a ValueError).

    Training: n_b ~ N(0, 1), sigma_b = exp(P_mean + P_std n_b), x = y + sigma_b eps, loss = mean_b mean_elem lambda(sigma_b)
    (D - y)^2.  Because lambda c_out^2 = 1 it is evaluated where it is best conditioned, as the plain MSE between the raw
    network output F and F* = (y - c_skip x) / c_out; the network sees c_in x and c_noise = (P_mean + P_std n_b) / 4.
    Sampling: Algorithm 2 on ``num_sample_steps`` levels of the rho-schedule, ``sampler="heun"`` (second order, two forwards a
    step but the last) or ``"euler"`` (first order, one forward a step); S_churn > 0 adds noise on the levels inside
    [S_tmin, S_tmax].  Class conditioning and classifier-free guidance as in ``GaussianDiffusion``: ``Unet(num_classes=K)``,
    ``cond_drop_prob`` in ``forward``, ``cond_scale`` per evaluation - mixing F is mixing D, the map is affine with the same
    coefficients for both.

    ``distill_from``, ``inpaint``, ``vlb_terms`` and ``encode`` do not exist here: they are built on the discrete-time chain."""

    def __init__(self, model: Unet, *, img_size, num_sample_steps=32, sigma_min=0.002, sigma_max=80.0, sigma_data=0.5,
                 rho=7.0, P_mean=-1.2, P_std=1.2, S_churn=0.0, S_tmin=0.05, S_tmax=50.0, S_noise=1.003, auto_normalize=True,
                 cond_drop_prob=None, cond_scale=1.0, sampler="heun"):
        super().__init__()
        if not getattr(model, "random_or_learned_sinusoidal_cond", False):
            raise ValueError("ElucidatedDiffusion needs a Unet built with learned_sinusoidal_cond=True or "
                             "random_fourier_features=True: the network reads the real-valued c_noise")
        plan.check_arguments(num_sample_steps, sigma_min, sigma_max, sigma_data, rho, P_std, S_churn)
        if sampler not in ("heun", "euler"):
            raise ValueError(f"sampler must be 'heun' or 'euler', got {sampler!r}")
        self.num_classes = getattr(model, "num_classes", None)
        if cond_drop_prob is None:
            cond_drop_prob = 0.1 if self.num_classes is not None else 0.0
        if not 0.0 <= float(cond_drop_prob) <= 1.0:
            raise ValueError(f"cond_drop_prob must lie in [0, 1], got {cond_drop_prob!r}")
        if self.num_classes is None and (float(cond_drop_prob) > 0.0 or float(cond_scale) != 1.0):
            raise ValueError("cond_drop_prob > 0 and cond_scale != 1 need a model built with num_classes")
        self.cond_drop_prob, self.cond_scale = float(cond_drop_prob), float(cond_scale)
        self.model, self.channels, self.img_size = model, model.channels, img_size
        self.num_sample_steps, self.sampler = int(num_sample_steps), sampler
        self.sigma_min, self.sigma_max, self.sigma_data, self.rho = float(sigma_min), float(sigma_max), float(sigma_data), float(rho)
        self.P_mean, self.P_std = float(P_mean), float(P_std)
        self.S_churn, self.S_tmin, self.S_tmax, self.S_noise = float(S_churn), float(S_tmin), float(S_tmax), float(S_noise)
        self.auto_normalize = auto_normalize
        # the loss is lgm_weighted_mse_fwd / _bwd over this one-entry weight table and an all-zero index tensor
        self.num_timesteps = 1
        self.register_buffer("loss_weight", torch.ones(1), persistent=False)
        self._zero_index = {}

    # -- the definitions on the host (float64) --------------------------------------------------------------------------
    def coefficients(self, sigma: float):
        """(c_in, c_noise, c_skip, c_out) at ``sigma``"""
        return plan.coefficients(float(sigma), self.sigma_data)

    def sample_schedule(self, steps=None):
        """the N + 1 levels sigma_0 = sigma_max ... sigma_{N-1} = sigma_min, sigma_N = 0"""
        return plan.sigma_grid(self.num_sample_steps if steps is None else steps, self.sigma_min, self.sigma_max, self.rho)

    def sample_plan(self, steps=None):
        """one row of ``lgm_hip.edm.ROW`` float64 values per step (``lgm_hip.edm.edm_plan``)"""
        return plan.edm_plan(self.num_sample_steps if steps is None else steps, sigma_min=self.sigma_min,
                             sigma_max=self.sigma_max, sigma_data=self.sigma_data, rho=self.rho, S_churn=self.S_churn,
                             S_tmin=self.S_tmin, S_tmax=self.S_tmax, S_noise=self.S_noise)

    # -- training -------------------------------------------------------------------------------------------------------
    def zero_index(self, B, device):
        """the all-zero int64 [B] index into the one-entry weight table, made once per (B, device)"""
        key = (B, torch.device(device))
        z = self._zero_index.get(key)
        if z is None:
            z = self._zero_index[key] = torch.zeros(B, dtype=torch.long, device=device)
        return z

    def draw(self, img, labels=None, *, t=None, sigma=None, noise=None, classes=None, dropout_key=None) -> StepDraws:
        """The random operands of a training step on the batch ``img``: what is given is used, the rest is drawn from torch's
        device generator in THIS order - n ~ randn(B) (``t`` of the record; not with ``sigma`` given), noise ~ randn_like(img),
        the label drop (``labels`` given and ``cond_drop_prob > 0``; ``classes``: the labels as the network gets them), the
        dropout key (``dropout > 0`` in training mode)."""
        B, dev = img.shape[0], img.device
        if t is None and sigma is None:
            t = torch.randn(B, device=dev)
        if noise is None:
            noise = torch.randn_like(img)
        classes = self.step_labels(labels, classes, B, dev)
        key = dropout_key if dropout_key is not None else self.draw_dropout_key(dev)
        return StepDraws(t, noise, None, classes, key, None)

    def qsample(self, img, d: StepDraws, normalize: bool, sigma=None) -> QSample:
        """``edm_loss_qsample`` from the batch and its draws (``d.t``: the normal draw n), or at the given ``sigma``"""
        return edm_loss_qsample(self, img, d.noise, normalize, d.t, sigma)

    def forward(self, img, classes=None):
        """The training loss of a batch in the data range; ``classes``: its labels, which go through the label drop"""
        b, c, h, w = img.shape
        assert h == self.img_size and w == self.img_size, f"height and width of image must be {self.img_size}"
        return self._loss_of(img, self.draw(img, classes), None, self.auto_normalize)

    def p_losses(self, img, sigma=None, noise=None, classes=None, *, _normalize=False, _dropout_key=None):
        """``img`` already normalised unless ``_normalize``.  ``sigma`` (float32 [B]) / ``noise`` / ``classes`` (the labels as
        the network gets them): explicit operands for parity tests; what is not given is drawn (``draw``) - sigma through its
        normal."""
        if sigma is not None:
            sigma = torch.as_tensor(sigma, dtype=torch.float32, device=img.device).reshape(-1).expand(img.shape[0]).contiguous()
        d = self.draw(img, None, sigma=sigma, noise=noise, classes=classes, dropout_key=_dropout_key)
        return self._loss_of(img, d, sigma, _normalize)

    def _loss_of(self, img, d: StepDraws, sigma, normalize):
        return self._loss(img, lambda save: edm_loss_forward(self, img, d.noise, d.t, sigma, bool(normalize), save, d.classes,
                                                             d.dropout_key))

    # -- the denoiser ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def preconditioned(self, x, sigma, classes=None, cond_scale=1.0, clip=False):
        """D(x, sigma) = c_skip x + c_out F(c_in x, c_noise) for NCHW ``x`` and ``sigma`` (a float, or one per sample) - the
        network on the HIP engine (guided: two forwards and the mix), the coefficients from float64 on the host.  An
        inspection call: the two scalings around the network are torch expressions, the samplers and the loss do not come
        through here."""
        b = x.shape[0]
        x = x.detach().to(self.device).float().contiguous()
        sig = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1).expand(b).tolist()
        co = torch.tensor([self.coefficients(s) for s in sig], dtype=torch.float64).to(torch.float32).to(self.device)
        c_in, c_noise, c_skip, c_out = (co[:, k].contiguous() for k in range(4))
        labels = self.model.labels(classes, b, self.device)
        if float(cond_scale) != 1.0 and self.num_classes is None:
            raise ValueError("cond_scale != 1 needs a model built with num_classes")
        self.model._anchor(self.device)
        F = self.model.run_nchw(x * c_in.view(b, 1, 1, 1), c_noise, False, None, labels, cond_scale)[0]
        D = c_skip.view(b, 1, 1, 1) * x + c_out.view(b, 1, 1, 1) * F
        return D.clamp_(-1.0, 1.0) if clip else D

    # -- sampling -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, batch_size=None, steps=None, classes=None, cond_scale=None, return_all_timesteps=False,
               clip_denoised=True, *, sampler=None, init_noise=None, noises=None):
        """Algorithm 2 from x_0 = sigma_0 noise -> [B, C, S, S] in the data range (clamped to [-1, 1], then unnormalised), or
        every state of the chain stacked along dim 1.  ``steps`` / ``sampler``: default the constructor's.  ``classes`` /
        ``cond_scale`` as in ``GaussianDiffusion.sample``.  ``clip_denoised``: D is clamped to [-1, 1] in both evaluations.
        A chain with S_churn > 0 draws one noise tensor per step (also on the steps whose gamma is zero, which do not read
        it: the captured step is one graph); ``init_noise`` / ``noises`` (one NCHW tensor per step) stand in for the draws in
        parity runs.  Replayed from captured steps (keys ``("edm", ...)``) unless every state is asked for."""
        B = 16 if batch_size is None else int(batch_size)
        kind = self.sampler if sampler is None else sampler
        if kind not in ("heun", "euler"):
            raise ValueError(f"sampler must be 'heun' or 'euler', got {kind!r}")
        scale = self.cond_scale if cond_scale is None else float(cond_scale)
        if classes is None:
            scale = 1.0
        if scale != 1.0 and self.num_classes is None:
            raise ValueError("cond_scale != 1 needs a model built with num_classes")
        dev = self.device
        labels = self.model.labels(classes, B, dev)
        rows = self.sample_plan(steps)
        shape = (B, self.channels, self.img_size, self.img_size)
        return _run_chain(self, shape, rows, kind == "heun", labels, scale, bool(clip_denoised), return_all_timesteps,
                          init_noise, noises)


def edm_loss_qsample(ed: ElucidatedDiffusion, img, noise, normalize: bool, n=None, sigma=None) -> QSample:
    """c_in x into the network's input buffer, F* into the target, sigma and c_noise per sample: one launch
    (``lgm_edm_qsample`` from the normal draw ``n``, ``lgm_edm_qsample_sigma`` from ``sigma``).  -> what ``hip_loss_network``
    reads: ``t`` the all-zero index into the one-entry weight table, ``net_t`` = c_noise; ``offset`` carries sigma [B]."""
    net = ed.model
    B, C, H, W = img.shape
    img = img.detach().float().contiguous()
    noise = noise.detach().float().contiguous()
    xin = net.input_buffer(B, H, W, img)
    target = ops.new((B, H, W, _r4(C)), img)
    sig, cn = ops.new((B,), img), ops.new((B,), img)
    ops.edm_qsample(img, noise, xin, net.x_off, target, sig, cn, ed.sigma_data, normalize, n=n, sigma=sigma, P_mean=ed.P_mean,
                    P_std=ed.P_std)
    return QSample(xin, target, img, noise, ed.zero_index(B, img.device), None, None, cn)


def edm_loss_forward(ed: ElucidatedDiffusion, img, noise, n, sigma, normalize: bool, save: bool, classes=None, dropout_key=None):
    """q_sample + UNet + MSE(F, F*) on the HIP engine -> (loss[1], ctx): ``hip_loss_network`` behind ``edm_loss_qsample``"""
    q = ed.qsample(img, StepDraws(n, noise, None, classes, dropout_key, None), normalize, sigma)
    return hip_loss_network(ed, q.xt, q.target, q.img, q.t, q.noise, q.offset, save, classes, normalize, dropout_key,
                            net_t=q.net_t)


# ----------------------------------------------------------------------------------------
# sampling: eager launches and the two captured steps
# ----------------------------------------------------------------------------------------
class _State:
    """The buffers of a chain: the unscaled sample state ``x``, ``xhat`` and ``d`` ([B, H, W, r4(C)] each), the network's input
    buffer ``xin`` (c_in x alone) and ``cnoise`` [B]."""

    def __init__(self, net, shape, dev):
        B, C, H, W = shape
        self.x, self.xhat, self.d = (torch.zeros((B, H, W, _r4(C)), device=dev) for _ in range(3))
        self.xin = torch.zeros((B, H, W, net.in_pitch), device=dev)
        self.cnoise = torch.zeros(B, device=dev)


def _step_launches(net, st: _State, C, second: bool, clip: bool, noise, classes, scale, scale_dev=None, row=None, table=None,
                   counter=None):
    """One step: pre -> forward -> euler [-> forward -> heun].  The row by value, or row ``counter`` of ``table`` with the
    counter advanced by the step's last launch.  Guided: two forwards and ``lgm_cfg_mix`` per evaluation."""
    kw = dict(row=row, table=table, counter=counter)
    adv = table is not None
    ops.edm_pre(st.x, noise, st.xhat, st.xin, net.x_off, st.cnoise, C, **kw)
    F = net.forward_guided(st.xin, st.cnoise, classes, scale, refresh_weights=False, scale_dev=scale_dev)
    ops.edm_euler(F, st.xhat, st.x, C, clip, d=st.d, xin=st.xin, x_off=net.x_off, cnoise=st.cnoise, second=second,
                  advance=adv and not second, **kw)
    if second:
        F = net.forward_guided(st.xin, st.cnoise, classes, scale, refresh_weights=False, scale_dev=scale_dev)
        ops.edm_heun(F, st.xhat, st.d, st.x, C, clip, advance=adv, **kw)


class _GraphedEdmStep(_CapturedStep):
    """One captured step of Algorithm 2 for a (network, batch shape, second evaluation or not, guided, clip, with noise);
    replayed once per step of any chain on it from the rows in ``table``.  A Heun chain is N - 1 replays of the step with the
    second evaluation and one of the step without."""

    def __init__(self, net, shape, second: bool, guided: bool, clip: bool, with_noise: bool, dev, max_steps: int = 1024):
        super().__init__(net, dev, max_steps, plan.ROW)
        B, C, H, W = shape
        self.state = _State(net, shape, dev)
        self.noise = torch.zeros(shape, device=dev) if with_noise else None
        self.classes = net.labels(None, B, dev).clone() if net.num_classes is not None else None
        self.scale = torch.ones(1, device=dev) if guided else None

        def one_step():
            nz = None
            if with_noise:
                nz = self.noise if self.inject else torch.randn(shape, device=dev)
            _step_launches(net, self.state, C, second, clip, nz, self.classes, 1.0, self.scale, table=self.table,
                           counter=self.counter)

        self._capture(one_step, (False, True) if with_noise else (False,), dev)

    def run(self, state: _State, rows, noises, classes, scale):
        """the steps ``rows`` from ``state.x`` -> ``state.x`` afterwards"""
        if self.classes is not None:
            self.classes.copy_(classes)
        if self.scale is not None:
            self.scale.fill_(float(scale))
        self.state.x.copy_(state.x)
        inject = noises is not None and self.noise is not None
        self._replay([0] * len(rows), rows, inject, None, (lambda i: self.noise.copy_(noises[i])) if inject else None)
        state.x.copy_(self.state.x)


def _graphed_step(ed, net, shape, second, guided, clip, with_noise):
    dev = ed.device
    key = ("edm", tuple(shape), bool(second), bool(guided), bool(clip), bool(with_noise))
    return _cached_step(net, key, lambda: _GraphedEdmStep(net, tuple(shape), second, guided, clip, with_noise, dev),
                        "elucidated sampler", dev)


def _run_chain(ed: ElucidatedDiffusion, shape, rows, heun: bool, classes, scale, clip, return_all, init_noise, noises):
    net, dev = ed.model, ed.device
    B, C, H, W = shape
    net.prepare_hip(dev)
    with_noise = any(r[plan.COEF] != 0.0 for r in rows) or ed.S_churn > 0.0
    if noises is not None and len(noises) != len(rows):
        raise ValueError(f"noises must hold one tensor per step ({len(rows)}), got {len(noises)}")
    if init_noise is None:
        init_noise = torch.randn(shape, device=dev)
    st = _State(net, shape, dev)
    # x_0 = sigma_0 noise: the level rounded once, one product per element
    x0 = init_noise.to(dev).float() * float(torch.tensor(rows[0][plan.S_I], dtype=torch.float64).to(torch.float32))
    ops.nchw_to_nhwc(x0.contiguous(), st.x)
    n = len(rows)
    seconds = [heun and rows[i][plan.S_NEXT] > 0.0 for i in range(n)]
    guided = scale != 1.0
    nz = None if noises is None else [None if v is None else v.to(dev).float().contiguous() for v in noises]

    def image():
        out = torch.empty(shape, device=dev)
        ops.nhwc_to_nchw(st.x[..., :C], out)
        return out

    imgs = [image()] if return_all else None
    i = 0
    while i < n:
        j = i
        while j < n and seconds[j] == seconds[i]:
            j += 1                                   # [i, j): steps of one kind - one captured step replays them all
        g = None if return_all else _graphed_step(ed, net, shape, seconds[i], guided, clip, with_noise)
        if g is not None:
            g.run(st, rows[i:j], None if nz is None or not with_noise else nz[i:j], classes, scale)
        else:
            net.refresh_derived_weights(False)
            for k in range(i, j):
                eps = None
                if with_noise:
                    eps = nz[k] if nz is not None else torch.randn(shape, device=dev)
                _step_launches(net, st, C, seconds[k], clip, eps, classes, scale, row=rows[k])
                if return_all:
                    imgs.append(image())
        i = j
    if return_all:
        out = torch.stack(imgs, dim=1)
    else:
        out = image()
    ops.clamp_(out, -1.0, 1.0)
    return ed.unnormalize(out)


# ----------------------------------------------------------------------------------------
# LightningModule
# ----------------------------------------------------------------------------------------
class EDM(DiffusionModule):
    """``DDPM``'s training surface around ``ElucidatedDiffusion``: the same EMA (keys ``ema.online_model.*`` /
    ``ema.ema_model.*``), optimizer, logging and graph-replayed step (``make_fast_step``); ``sample`` samples under the EMA
    weights."""

    def __init__(self, img_channels: int = 3, img_size: int = 64, dim: int = 64, num_sample_steps: int = 32,
                 lr: float = 2e-5, betas: Tuple[float, float] = (0.9, 0.99), ema_update_every: int = 10,
                 ema_decay: float = 0.995, sigma_min: float = 0.002, sigma_max: float = 80.0, sigma_data: float = 0.5,
                 rho: float = 7.0, P_mean: float = -1.2, P_std: float = 1.2, S_churn: float = 0.0, S_tmin: float = 0.05,
                 S_tmax: float = 50.0, S_noise: float = 1.003, sampler: str = "heun", learned_sinusoidal_cond: bool = True,
                 random_fourier_features: bool = False, learned_sinusoidal_dim: int = 16, num_classes: Optional[int] = None,
                 cond_drop_prob: float = 0.1, cond_scale: float = 1.0, dropout: float = 0.0):
        super().__init__()
        self.save_hyperparameters()
        self.num_classes = num_classes
        model = Unet(dim=dim, channels=img_channels, learned_sinusoidal_cond=learned_sinusoidal_cond,
                     random_fourier_features=random_fourier_features, learned_sinusoidal_dim=learned_sinusoidal_dim,
                     num_classes=num_classes, dropout=dropout)
        cond = dict(cond_drop_prob=cond_drop_prob, cond_scale=cond_scale) if num_classes is not None else {}
        diffusion = ElucidatedDiffusion(model, img_size=img_size, num_sample_steps=num_sample_steps, sigma_min=sigma_min,
                                        sigma_max=sigma_max, sigma_data=sigma_data, rho=rho, P_mean=P_mean, P_std=P_std,
                                        S_churn=S_churn, S_tmin=S_tmin, S_tmax=S_tmax, S_noise=S_noise, sampler=sampler, **cond)
        self.lowres_cond = False
        self._wrap(diffusion, img_channels, img_size, ema_decay, ema_update_every)

    @torch.no_grad()
    def _log_sample(self):
        kw = {}
        if self.num_classes is not None:             # every class in turn, at the configured guidance scale
            kw["classes"] = torch.arange(64, device=self.ema.ema_model.device) % self.num_classes
        self.last_samples = self.sample(batch_size=64, **kw)
        self._log_images()

    @torch.no_grad()
    def sample(self, *a, **kw):
        """``ElucidatedDiffusion.sample`` under the EMA weights"""
        return self._shadow().sample(*a, **kw)
