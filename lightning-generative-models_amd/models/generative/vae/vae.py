"""MLP VAE - drop-in for the reference's models/generative/vae/vae.py:21-215: same class names, constructor arguments,
state_dict keys, losses (L1 reconstruction + kld_weight * KLD) and optimiser.

On a CPU device it is plain torch (autograd, ``torch.optim.Adam``): BASELINE config 1, the run that proves the train.py /
config / trainer wiring.  On a GPU device it rides the HIP engine like every other model: one flat parameter buffer, the
layers on the dense kernels of csrc/dense.hip (bias and LeakyReLU / tanh in the epilogue, the activation's derivative read
from the saved output), both latent heads with the reparameterisation and the KL terms in one launch, tanh + L1 in one
launch, ``training_step`` one autograd.Function over those launch sequences, ``FusedAdam`` and the graph-replayed
``ModuleFastStep``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from lgm_hip import ops
from lgm_hip.flat import FlatParams, _r4
from lgm_hip.lightning import LightningModule, multi_rank
from lgm_hip.nn import GradCtx, Linear, param_kind
from lgm_hip.optim import FusedAdam

SLOPE = 0.2


def _no_tape(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


class Encoder(nn.Module):
    """reference vae.py:21-56"""

    def __init__(self, img_channels, img_size, latent_dim):
        super().__init__()
        n = img_channels * img_size * img_size
        self.latent_dim = latent_dim
        self.layers = nn.Sequential(Linear(n, 512), nn.LeakyReLU(SLOPE), Linear(512, 256), nn.LeakyReLU(SLOPE),
                                    Linear(256, 128), nn.LeakyReLU(SLOPE))
        self.mu = Linear(128, latent_dim)
        self.log_var = Linear(128, latent_dim)

    def forward(self, x):
        h = self.layers(x.flatten(1))
        return self.mu(h), self.log_var(h)

    # ---- HIP engine: x2 [B, C S S] is the image batch's own memory -------------------------------------------------------
    def fwd(self, x2, eps):
        """-> (mu, log_var, z [B, r4(L)], kld_part [B]), saved activations"""
        acts = [x2]
        for i in (0, 2, 4):
            acts.append(self.layers[i].fwd(acts[-1], ops.ACT_LRELU, SLOPE))      # Linear -> LeakyReLU: one launch
        fp = self.mu.weight._lgm_flat
        mu, lv, z, part = ops.vae_head_fwd(acts[-1], 128, self.latent_dim, fp.ptr(self.mu.weight), fp.ptr(self.mu.bias),
                                           fp.ptr(self.log_var.weight), fp.ptr(self.log_var.bias), eps)
        return (mu, lv, z, part), acts

    def bwd(self, gc: GradCtx, acts, mu, lv, eps, gz, gloss, kld_weight: float):
        fp = gc.flat
        h = acts[3]
        beta = gc.beta(self.mu.weight)
        for p in (self.mu.bias, self.log_var.weight, self.log_var.bias):
            assert gc.beta(p) == beta
        g = ops.new(h.shape, h)
        ops.vae_head_bwd(gz, mu, lv, eps, gloss, kld_weight, h, 128, self.latent_dim, fp.ptr(self.mu.weight),
                         fp.ptr(self.log_var.weight), g, fp.gptr(self.mu.weight), fp.gptr(self.mu.bias),
                         fp.gptr(self.log_var.weight), fp.gptr(self.log_var.bias), beta)
        for k, i in ((3, 4), (2, 2), (1, 0)):
            g = self.layers[i].bwd(gc, acts[k - 1], acts[k], g, ops.ACT_LRELU, SLOPE, need_gx=(i != 0))


class Decoder(nn.Module):
    """reference vae.py:59-97"""

    def __init__(self, img_channels, img_size, latent_dim):
        super().__init__()
        self.shape = (img_channels, img_size, img_size)
        self.latent_dim = latent_dim
        sizes = [latent_dim, 128, 256, 512, math.prod(self.shape)]
        layers = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            layers += [Linear(a, b), nn.LeakyReLU(SLOPE)]
        layers[-1] = nn.Tanh()
        self.layers = nn.Sequential(*layers)

    def forward(self, z):
        return self.layers(z).view(-1, *self.shape)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def random_sample(self, batch_size: int):
        return self(torch.randn([batch_size, self.latent_dim], device=self.device))

    # ---- HIP engine -----------------------------------------------------------------------------------------------------
    def fwd(self, z, last_act=ops.ACT_NONE):
        """z [B, >= L] -> the last layer's output [B, r4(D)] (before the Tanh unless last_act says otherwise), saved acts"""
        acts = [z]
        for i in (0, 2, 4):
            acts.append(self.layers[i].fwd(acts[-1], ops.ACT_LRELU, SLOPE))
        return self.layers[6].fwd(acts[-1], last_act), acts

    def bwd(self, gc: GradCtx, acts, gpre):
        """gpre: gradient at the last layer's output BEFORE the Tanh -> gz [B, r4(L)]"""
        g = self.layers[6].bwd(gc, acts[3], None, gpre)
        for k, i in ((3, 4), (2, 2), (1, 0)):
            g = self.layers[i].bwd(gc, acts[k - 1], acts[k], g, ops.ACT_LRELU, SLOPE)
        return g


class VAE(LightningModule):
    def __init__(self, img_channels: int, img_size: int, latent_dim: int = 20, lr: float = 1e-4, b1: float = 0.9,
                 b2: float = 0.999, weight_decay: float = 1e-5, kld_weight: float = 1e-2):
        super().__init__()
        self.save_hyperparameters()
        self.encoder = Encoder(img_channels, img_size, latent_dim)
        self.decoder = Decoder(img_channels, img_size, latent_dim)
        self._flat: Optional[FlatParams] = None

    # ---- flat storage (GPU devices only) ---------------------------------------------------------------------------------
    def prepare_hip(self, device) -> Optional[FlatParams]:
        device = torch.device(device)
        if device.type != "cuda":
            return None                  # the CPU model stays plain torch: ordinary parameters, per-parameter .grad
        if self._flat is not None and self._flat.device == device and self._flat.still_bound():
            return self._flat
        named = [(n, p, param_kind(n, p)) for n, p in self.named_parameters()]
        self._flat = FlatParams(named, device)
        return self._flat

    def _on_hip(self, t: torch.Tensor) -> bool:
        if t.device.type != "cuda":
            return False
        self.prepare_hip(t.device)
        return True

    def _anchor(self, device):
        a = getattr(self, "_anchor_t", None)
        if a is None or a.device != torch.device(device):
            a = torch.zeros(1, device=device, requires_grad=True)
            self._anchor_t = a
        return a

    # ---- engine ---------------------------------------------------------------------------------------------------------
    def _dims(self):
        hp = self.hparams
        return hp.img_channels * hp.img_size * hp.img_size, hp.latent_dim

    def run(self, x: torch.Tensor, eps: torch.Tensor, save: bool):
        """x [B, C, S, S], eps [B, L] -> (vals3 = (loss, recon, kld), x_hat [B, r4(D)], mu, log_var), tape"""
        D, L = self._dims()
        B = x.shape[0]
        x2 = x.view(B, D)
        (mu, lv, z, kpart), enc_acts = self.encoder.fwd(x2, eps)
        pre, dec_acts = self.decoder.fwd(z)
        xh = ops.new(pre.shape, pre)
        rpart = ops.new((B,), pre)
        ops.tanh_l1_fwd(pre, x2, D, xh, rpart)
        vals = ops.new((3,), pre)
        ops.vae_loss(rpart, kpart, D, L, float(self.hparams.kld_weight), vals)
        tape = (x2, eps, enc_acts, mu, lv, dec_acts, xh) if save else None
        return (vals, xh, mu, lv), tape

    def backward_hip(self, tape, gloss):
        """gloss: device scalar d L / d loss; writes the flat gradient buffer"""
        x2, eps, enc_acts, mu, lv, dec_acts, xh = tape
        D, _ = self._dims()
        gc = GradCtx(self._flat)                 # refreshes the transposed weight copies the input gradients read
        gpre = ops.new(xh.shape, xh)
        ops.tanh_l1_bwd(xh, x2, gloss, D, gpre)
        gz = self.decoder.bwd(gc, dec_acts, gpre)
        self.encoder.bwd(gc, enc_acts, mu, lv, eps, gz, gloss, float(self.hparams.kld_weight))
        gc.flush()
        self._flat.bind_grad_views()

    def _image(self, xh: torch.Tensor) -> torch.Tensor:
        D, _ = self._dims()
        return xh[:, :D].reshape(-1, *self.decoder.shape)

    def _draw_eps(self, x: torch.Tensor) -> torch.Tensor:
        return torch.randn([x.shape[0], self.hparams.latent_dim], device=x.device)

    # ---- the reference's surface ----------------------------------------------------------------------------------------
    def reparameterize(self, mu, log_var):
        return mu + torch.randn_like(mu) * torch.exp(log_var / 2)

    def forward(self, x):
        if self._on_hip(x):
            _, L = self._dims()
            x = _no_tape(x)
            (_, xh, mu, lv), _ = self.run(x, self._draw_eps(x), False)
            return self._image(xh), mu[:, :L], lv[:, :L]
        mu, log_var = self.encoder(x)
        return self.decoder(self.reparameterize(mu, log_var)), mu, log_var

    def _common_step(self, batch, batch_idx, split):
        x, _ = batch
        if self._on_hip(x):
            loss, recon, kld = _VAEStepFn.apply(self._anchor(x.device), self, x)
            self.log_dict({f"{split}_loss": loss, f"{split}_recon_loss": recon, f"{split}_kld": kld}, prog_bar=True,
                          logger=True, sync_dist=multi_rank())
            return loss
        x_hat, mu, log_var = self(x)
        recon = torch.nn.functional.l1_loss(x_hat, x)
        kld = -0.5 * torch.mean(1 + log_var - mu.pow(2) - log_var.exp())
        loss = recon + self.hparams.kld_weight * kld
        self.log_dict({f"{split}_loss": loss, f"{split}_recon_loss": recon, f"{split}_kld": kld})
        return loss

    def training_step(self, batch, batch_idx):
        return self._common_step(batch, batch_idx, "train")

    def validation_step(self, batch, batch_idx):
        if batch[0].device.type == "cuda":
            with torch.no_grad():                # the same forward, no tape
                return self._common_step(batch, batch_idx, "val")
        return self._common_step(batch, batch_idx, "val")

    def configure_optimizers(self):
        hp = self.hparams
        if self._flat is not None:
            return FusedAdam(self.parameters(), lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)
        return torch.optim.Adam(self.parameters(), lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)

    def make_fast_step(self, opt, world: int = 1, use_graph: bool = True, accumulate: int = 1):
        """The step object ``MiniTrainer.fit`` drives: training_step + backward replayed from one HIP graph (the draw of eps
        included), eager fallback inside."""
        from lgm_hip.graph import ModuleFastStep
        self.prepare_hip(next(self.parameters()).device)
        if self._flat is None:
            raise RuntimeError("make_fast_step needs the model on a GPU device")
        return ModuleFastStep(self, opt, world, use_graph, accumulate=accumulate)

    # ---- inference: both devices; launch sequences without a tape on the GPU ----------------------------------------------
    @torch.no_grad()
    def encode(self, x: torch.Tensor):
        """x [B, C, S, S] -> (mu, log_var) [B, latent_dim]"""
        if not self._on_hip(x):
            return self.encoder(x)
        _, L = self._dims()
        x = _no_tape(x)
        B = x.shape[0]
        (mu, lv, _, _), _ = self.encoder.fwd(x.view(B, -1), torch.zeros([B, L], device=x.device))
        return mu[:, :L], lv[:, :L]

    def _check_z(self, z: torch.Tensor):
        L = self.hparams.latent_dim
        if z.dim() != 2 or z.shape[1] != L:
            raise ValueError(f"z must be [n, {L}] (latent_dim), got {tuple(z.shape)}")

    @torch.no_grad()
    def decode(self, z: torch.Tensor):
        """z [n, latent_dim] -> images [n, C, S, S] in (-1, 1)"""
        self._check_z(z)
        if not self._on_hip(z):
            return self.decoder(z)
        xh, _ = self.decoder.fwd(_no_tape(z), ops.ACT_TANH)
        return self._image(xh)

    @torch.no_grad()
    def reconstruct(self, x: torch.Tensor):
        """decode(mu(x)): the reconstruction at the posterior mean"""
        return self.decode(self.encode(x)[0])

    @torch.no_grad()
    def sample(self, num_samples: int, z: Optional[torch.Tensor] = None):
        """decode(z ~ N(0, I)) (the reference's Decoder.random_sample); ``z`` [num_samples, latent_dim] replaces the draw"""
        L = self.hparams.latent_dim
        if z is None:
            z = torch.randn([num_samples, L], device=self.decoder.device)
        self._check_z(z)
        if z.shape[0] != num_samples:
            raise ValueError(f"z must be [{num_samples}, {L}], got {tuple(z.shape)}")
        return self.decode(z)


class _VAEStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, m: VAE, x):
        ctx.set_materialize_grads(False)
        save = bool(ctx.needs_input_grad[0])
        x = _no_tape(x)
        eps = m._draw_eps(x)                         # from the device generator, inside the step: captured with it
        (vals, _, _, _), tape = m.run(x, eps, save)
        ctx.stuff = (m, tape)
        loss, recon, kld = vals[0], vals[1], vals[2]
        ctx.mark_non_differentiable(recon, kld)
        return loss, recon, kld

    @staticmethod
    def backward(ctx, gloss, *_unused):
        m, tape = ctx.stuff
        if tape is None:
            raise RuntimeError("VAE step ran without saving activations")
        m.backward_hip(tape, gloss.detach().float().reshape(1).contiguous())
        ctx.stuff = None
        return None, None, None
