"""GAN base LightningModule and the reference's MLP GAN - drop-in for models/generative/gan/gan.py: the same class names,
constructor arguments, state_dict keys, losses (reference :258-308) and optimisers.

``GAN`` is the base of DCGAN / LSGAN / R1GAN / WGAN (manual optimisation, two Adam optimisers, the alternating
_common_step); those subclasses build their own convolutional ``G`` / ``D``.  Constructed on its own it is the reference's
MLP GAN: ``Generator`` (Linear -> BatchNorm1d -> LeakyReLU three times, Linear -> Tanh) against ``Discriminator`` (a
three-layer MLP).

On a CPU device both networks are plain torch (autograd, ``torch.optim.Adam``).  On a GPU device each rides the HIP engine:
one flat parameter buffer per network, the layers on the dense kernels of csrc/dense.hip and the one-launch BatchNorm1d of
csrc/bn1d.hip behind autograd.Functions (activation derivatives read from saved outputs), the binary cross entropy on the
critic logits one launch forward and one backward, an input-gradient-only sweep through ``D`` for the generator update,
``FusedAdam`` and the graph-replayed ``GANFastStep``.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
from torch import nn

from lgm_hip import ops
from lgm_hip.bn import BatchNorm1d
from lgm_hip.flat import FlatParams
from lgm_hip.lightning import LightningModule, multi_rank
from lgm_hip.nn import GradCtx, Linear, param_kind
from lgm_hip.optim import FusedAdam

SLOPE = 0.2
LOSS_TYPES = ("non-saturating", "min-max")


def _rows2d(t: torch.Tensor) -> torch.Tensor:
    """[B, ...] -> the [B, n] float32 rows the dense kernels read, without a copy where the memory allows (an NCHW batch, the
    generator's padded output seen as images)"""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    t2 = t.reshape(t.shape[0], -1)
    if t2.shape[1] > 1 and t2.stride(1) != 1 or t2.shape[0] > 1 and t2.stride(0) < t2.shape[1]:
        t2 = t2.contiguous()
    if t2.shape[0] == 1 and t2.stride(0) < t2.shape[1]:
        t2 = t2.contiguous()
    return t2


class _MLPNet(nn.Module):
    """Flat-storage plumbing of the two MLPs: nothing on a CPU device, one FlatParams on a GPU device."""

    def __init__(self):
        super().__init__()
        self._flat: Optional[FlatParams] = None

    def prepare_hip(self, device) -> Optional[FlatParams]:
        device = torch.device(device)
        if device.type != "cuda":
            return None                  # the CPU network stays plain torch: ordinary parameters, per-parameter .grad
        if self._flat is not None and self._flat.device == device and self._flat.still_bound():
            return self._flat
        self._flat = FlatParams([(n, p, param_kind(n, p)) for n, p in self.named_parameters()], device)
        return self._flat

    def _on_hip(self, t: torch.Tensor) -> bool:
        if t.device.type != "cuda":
            return False
        self.prepare_hip(t.device)
        return True

    def _anchor(self, device):
        self.prepare_hip(device)
        a = getattr(self, "_anchor_t", None)
        if a is None or a.device != torch.device(device):
            a = torch.zeros(1, device=device, requires_grad=True)
            self._anchor_t = a
        return a

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device


class Generator(_MLPNet):
    """reference gan.py:15-58"""

    def __init__(self, img_channels: int, img_size: int, latent_dim: int):
        super().__init__()
        self.img_shape = [img_channels, img_size, img_size]
        self.latent_dim = latent_dim
        self.model = nn.Sequential(
            Linear(latent_dim, 256), BatchNorm1d(256), nn.LeakyReLU(SLOPE),
            Linear(256, 512), BatchNorm1d(512), nn.LeakyReLU(SLOPE),
            Linear(512, 1024), BatchNorm1d(1024), nn.LeakyReLU(SLOPE),
            Linear(1024, math.prod(self.img_shape)), nn.Tanh())

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        if self._on_hip(z):
            return _GenFn.apply(self._anchor(z.device), self, z)
        return self.model(z).view(-1, *self.img_shape)

    def random_sample(self, batch_size: int) -> torch.Tensor:
        z = torch.randn([batch_size, self.latent_dim], device=self.device)
        return self(z)

    # ---- HIP engine -----------------------------------------------------------------------------------------------------
    def image(self, xh: torch.Tensor) -> torch.Tensor:
        """the padded output [B, r4(D)] seen as images [B, C, S, S]: a view"""
        return xh[:, :math.prod(self.img_shape)].view(-1, *self.img_shape)

    def fwd(self, z, save: bool = True):
        """z [B, >= latent_dim] -> x_hat [B, r4(D)] (pad lanes 0), tape[k] = (layer input, BatchNorm saved, layer output)"""
        h, tape = z, []
        for i in (0, 3, 6):
            a = self.model[i].fwd(h, ops.ACT_NONE)
            hn, sv = self.model[i + 1].fwd(a, ops.ACT_LRELU, SLOPE, self.training)     # BatchNorm -> LeakyReLU: one launch
            tape.append((h, sv, hn))
            h = hn
        xh = self.model[9].fwd(h, ops.ACT_TANH)
        tape.append((h, None, xh))
        return xh, (tape if save else None)

    def bwd(self, tape, gout):
        """gout [B, >= D]: gradient at x_hat; tanh' and LeakyReLU' are read from the saved outputs"""
        gc = GradCtx(self._flat)                 # refreshes the transposed weight copies the input gradients read
        h, _, xh = tape[3]
        g = self.model[9].bwd(gc, h, xh, gout, ops.ACT_TANH)
        for k, i in ((2, 6), (1, 3), (0, 0)):
            h_in, sv, hn = tape[k]
            ga = self.model[i + 1].bwd(gc, sv, hn, g, ops.ACT_LRELU, SLOPE)
            g = self.model[i].bwd(gc, h_in, None, ga, ops.ACT_NONE, need_gx=(i != 0))
        gc.flush()
        self._flat.bind_grad_views()


class _GenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, net: Generator, z):
        save = bool(ctx.needs_input_grad[0])
        xh, tape = net.fwd(_rows2d(z), save)
        ctx.net, ctx.tape = net, tape
        return net.image(xh)

    @staticmethod
    def backward(ctx, gy):
        if ctx.tape is None:
            raise RuntimeError("Generator forward ran without saving activations")
        ctx.net.bwd(ctx.tape, _rows2d(gy))
        ctx.tape = None
        return None, None, None


class Discriminator(_MLPNet):
    """reference gan.py:61-89"""

    def __init__(self, img_channels: int, img_size: int):
        super().__init__()
        n = img_channels * img_size * img_size
        self.model = nn.Sequential(Linear(n, 512), nn.LeakyReLU(SLOPE), Linear(512, 256), nn.LeakyReLU(SLOPE), Linear(256, 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._on_hip(x):
            return _DiscFn.apply(self._anchor(x.device), self, x)
        return self.model(x.view(x.size(0), -1)).squeeze()

    # ---- HIP engine: x2 [B, >= C S S] is the image batch's own memory, or the generator's padded output ---------------------
    def fwd(self, x2):
        """-> scores [B, 4] (column 0), tape"""
        a1 = self.model[0].fwd(x2, ops.ACT_LRELU, SLOPE)
        a2 = self.model[2].fwd(a1, ops.ACT_LRELU, SLOPE)
        s = self.model[4].fwd(a2, ops.ACT_NONE)
        return s, (x2, a1, a2)

    def bwd(self, gc: GradCtx, tape, gs, need_gx: bool = False):
        """gs [B, 4] (column 0): parameter gradients into the flat buffer; returns the input gradient when asked"""
        x2, a1, a2 = tape
        g = self.model[4].bwd(gc, a2, None, gs, ops.ACT_NONE)
        g = self.model[2].bwd(gc, a1, a2, g, ops.ACT_LRELU, SLOPE)
        return self.model[0].bwd(gc, x2, a1, g, ops.ACT_LRELU, SLOPE, need_gx=need_gx)

    def bwd_input(self, tape, gs):
        """The input gradient alone [B, r4(C S S)]: the generator update's sweep - no parameter gradient of D is formed"""
        _, a1, a2 = tape
        self._flat.refresh_transposed()          # the weights moved since the last backward pass (d_optim.step())
        g = self.model[4].dgrad(None, gs, ops.ACT_NONE)
        g = self.model[2].dgrad(a2, g, ops.ACT_LRELU, SLOPE)
        return self.model[0].dgrad(a1, g, ops.ACT_LRELU, SLOPE)


class _DiscFn(torch.autograd.Function):
    """logits = D(x).squeeze(); backward gives parameter gradients and (if needed) dL/dx"""

    @staticmethod
    def forward(ctx, anchor, net: Discriminator, x):
        s, tape = net.fwd(_rows2d(x))
        save = bool(ctx.needs_input_grad[0]) or bool(ctx.needs_input_grad[2])
        ctx.net, ctx.tape, ctx.shape = net, (tape if save else None), x.shape
        return s[:, 0].clone().squeeze()

    @staticmethod
    def backward(ctx, gs):
        net = ctx.net
        if ctx.tape is None:
            raise RuntimeError("Discriminator forward ran without saving activations")
        B = ctx.shape[0]
        g4 = torch.zeros((B, 4), device=gs.device)
        g4[:, 0] = gs.reshape(B)
        need_x = bool(ctx.needs_input_grad[2])
        if ctx.needs_input_grad[0]:
            gc = GradCtx(net._flat)
            gx = net.bwd(gc, ctx.tape, g4, need_x)
            gc.flush()
            net._flat.bind_grad_views()
        else:
            gx = net.bwd_input(ctx.tape, g4)
        ctx.tape = None
        n = math.prod(ctx.shape[1:])
        return None, None, (gx[:, :n].view(ctx.shape) if need_x else None)


class _DLossFn(torch.autograd.Function):
    """reference :258-283 as one Function: D on the real and on the fake batch, the five logged values in one launch; the
    backward writes the score gradients in one launch and runs D's backward twice into the flat gradient buffer"""

    @staticmethod
    def forward(ctx, anchor, D: Discriminator, x, x_hat):
        ctx.set_materialize_grads(False)
        save = bool(ctx.needs_input_grad[0])
        s_real, t_real = D.fwd(_rows2d(x))
        s_fake, t_fake = D.fwd(_rows2d(x_hat))
        vals = ops.gan_bce_d(s_real, s_fake, ops.new((5,), s_real))
        ctx.stuff = (D, s_real, t_real, s_fake, t_fake) if save else None
        outs = (vals[2], vals[0], vals[1], vals[3], vals[4])
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(ctx, gloss, *_unused):
        if ctx.stuff is None:
            raise RuntimeError("the discriminator loss ran without saving activations")
        D, s_real, t_real, s_fake, t_fake = ctx.stuff
        gl = gloss.detach().float().reshape(1).contiguous()
        gc = GradCtx(D._flat)
        g_real, g_fake = ops.new(s_real.shape, s_real), ops.new(s_fake.shape, s_fake)
        ops.gan_bce_bwd(gl, s_real, 1.0, 0.5, g_real, s_fake, 0.0, 0.5, g_fake)
        D.bwd(gc, t_real, g_real)
        D.bwd(gc, t_fake, g_fake)
        gc.flush()
        D._flat.bind_grad_views()
        ctx.stuff = None
        return None, None, None, None


class _GLossFn(torch.autograd.Function):
    """reference :285-308: (g_loss, mean logit) from D(x_hat); the backward returns d g_loss / d x_hat only (D's own parameter
    gradients of this pass are discarded by the reference's next zero_grad anyway)"""

    @staticmethod
    def forward(ctx, D: Discriminator, x_hat, loss_type: str):
        ctx.set_materialize_grads(False)
        D.prepare_hip(x_hat.device)
        s, tape = D.fwd(_rows2d(x_hat))
        vals = ops.gan_bce_g(s, loss_type, ops.new((2,), s))
        ctx.stuff = (D, s, tape, x_hat.shape, loss_type) if ctx.needs_input_grad[1] else None
        ctx.mark_non_differentiable(vals[1])
        return vals[0], vals[1]

    @staticmethod
    def backward(ctx, gloss, *_unused):
        if ctx.stuff is None:
            raise RuntimeError("the generator loss ran without saving activations")
        D, s, tape, shape, loss_type = ctx.stuff
        gl = gloss.detach().float().reshape(1).contiguous()
        g = ops.new(s.shape, s)
        if loss_type == "non-saturating":
            ops.gan_bce_bwd(gl, s, 1.0, 1.0, g)          # d bce(s, 1)
        else:
            ops.gan_bce_bwd(gl, s, 0.0, -1.0, g)         # d -bce(s, 0)
        gx = D.bwd_input(tape, g)
        ctx.stuff = None
        return None, gx[:, :math.prod(shape[1:])].view(shape), None


class GAN(LightningModule):
    def __init__(self, img_channels: int = 1, img_size: int = 28, latent_dim: int = 100, lr: float = 1e-4,
                 b1: float = 0.5, b2: float = 0.999, weight_decay: float = 1e-5, loss_type: str = "non-saturating",
                 calculate_metrics: bool = False, metrics: List[str] = [], summary: bool = True):
        super().__init__()
        self.save_hyperparameters()
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
        self.automatic_optimization = False      # reference gan.py:118
        self.calculate_metrics = calculate_metrics
        self.metrics = metrics
        self.G = None
        self.D = None
        if type(self) is GAN:
            # the reference's MLP pair (gan.py:122-137).  The subclasses build their own networks: nothing is constructed
            # or drawn for them here, so their initial weights for a seed are what they were
            self.G = Generator(img_channels=img_channels, img_size=img_size, latent_dim=latent_dim)
            self.D = Discriminator(img_channels=img_channels, img_size=img_size)
            self.z = torch.randn([64, latent_dim])

    def _is_mlp(self) -> bool:
        return isinstance(self.G, Generator) and isinstance(self.D, Discriminator)

    def prepare_hip(self, device):
        self.G.prepare_hip(device)
        self.D.prepare_hip(device)

    def forward(self, z):
        return self.G(z)

    def _common_step(self, batch, mode: str):
        """reference gan.py:144-174: one D update then one G update per batch."""
        x, _ = batch
        x_hat = self.G.random_sample(x.size(0))
        d_optim, g_optim = self.optimizers()
        loss_dict = self._calculate_d_loss(x, x_hat)
        if self.training:
            d_optim.zero_grad(set_to_none=True)
            self.manual_backward(loss_dict["d_loss"])
            d_optim.step()
        loss_dict.update(self._calculate_g_loss(x_hat))
        if self.training:
            g_optim.zero_grad(set_to_none=True)
            self.manual_backward(loss_dict["g_loss"])
            g_optim.step()
        loss_dict = {f"{mode}_{k}": v for k, v in loss_dict.items()}
        self.log_dict(loss_dict, prog_bar=True, logger=True, sync_dist=multi_rank())
        return x, x_hat, loss_dict

    def training_step(self, batch):
        _, _, loss_dict = self._common_step(batch, "train")
        return loss_dict

    def validation_step(self, batch):
        self._common_step(batch, "val")

    def configure_optimizers(self):
        """reference gan.py:243-256: ([d_optim, g_optim], [])"""
        kw = dict(lr=self.hparams.lr, betas=(self.hparams.b1, self.hparams.b2), weight_decay=self.hparams.weight_decay)
        if self._is_mlp() and self.G._flat is None:
            return [torch.optim.Adam(self.D.parameters(), **kw), torch.optim.Adam(self.G.parameters(), **kw)], []
        return [FusedAdam(self.D.parameters(), **kw), FusedAdam(self.G.parameters(), **kw)], []

    def make_fast_step(self, opts, world: int = 1, use_graph: bool = True):
        """The step object ``MiniTrainer.fit`` drives instead of ``training_step`` for the MLP pair on a GPU device: the work
        in front of and behind the D optimizer step replayed from two HIP graphs (lgm_hip.graph.GANFastStep).  None for every
        other pair of networks (DCGAN / LSGAN / R1GAN): those models train through ``training_step`` as they did."""
        if not self._is_mlp():
            return None
        from lgm_hip.graph import GANFastStep
        self.prepare_hip(self.G.device)
        if self.G._flat is None or self.D._flat is None:
            raise RuntimeError("make_fast_step needs the model on a GPU device")
        return GANFastStep(self, opts, world, use_graph)

    # ---- the losses of the MLP pair (the subclasses override both) ---------------------------------------------------------
    def _calculate_d_loss(self, x, x_hat):
        """reference :258-283"""
        if self.D._on_hip(x):
            d_loss, real, fake, lr, lf = _DLossFn.apply(self.D._anchor(x.device), self.D, x, x_hat.detach())
            return {"d_loss": d_loss, "d_loss_real": real, "d_loss_fake": fake, "logits_real": lr, "logits_fake": lf}
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        logits_real = self.D(x)
        d_loss_real = bce(logits_real, torch.ones_like(logits_real))
        logits_fake = self.D(x_hat.detach())
        d_loss_fake = bce(logits_fake, torch.zeros_like(logits_fake))
        d_loss = (d_loss_real + d_loss_fake) / 2
        return {"d_loss": d_loss, "d_loss_real": d_loss_real, "d_loss_fake": d_loss_fake,
                "logits_real": logits_real.mean(), "logits_fake": logits_fake.mean()}

    def _calculate_g_loss(self, x_hat):
        """reference :285-308"""
        if self.D._on_hip(x_hat):
            g_loss, lf = _GLossFn.apply(self.D, x_hat, self.hparams.loss_type)
            return {"g_loss": g_loss, "logits_fake": lf}
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        logits_fake = self.D(x_hat)
        if self.hparams.loss_type == "min-max":
            g_loss = -bce(logits_fake, torch.zeros_like(logits_fake))
        else:
            g_loss = bce(logits_fake, torch.ones_like(logits_fake))
        return {"g_loss": g_loss, "logits_fake": logits_fake.mean()}

    @torch.no_grad()
    def sample(self, num_samples: int, z: Optional[torch.Tensor] = None):
        """G(z ~ N(0, I)) without a tape, in the module's current mode (train: batch statistics, and the running statistics
        move as in any train-mode forward; eval: running statistics); ``z`` [num_samples, latent_dim] replaces the draw"""
        if not self._is_mlp():
            raise NotImplementedError(f"{type(self).__name__}.sample: only the MLP pair of the base GAN")
        L = self.hparams.latent_dim
        if z is None:
            z = torch.randn([num_samples, L], device=self.G.device)
        if z.dim() != 2 or tuple(z.shape) != (num_samples, L):
            raise ValueError(f"z must be [{num_samples}, {L}] (num_samples, latent_dim), got {tuple(z.shape)}")
        return self.G(z)
