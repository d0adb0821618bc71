"""Denoising autoencoder - drop-in for the reference's models/generative/autoencoder/dae.py: same class names, constructor
arguments, state_dict keys (``encoder.model.{0,2}``, ``decoder.model.{0,2}``), corruption (Gaussian, salt-and-pepper), MSE
loss against the clean batch and optimiser (Adam, lr 1e-3).  Beyond the reference: the input width is
``img_channels * img_size^2`` instead of a fixed 784, ``noise_type="masking"`` (every element becomes 0 with probability
``noise_level``), the optimiser's hyperparameters, and the inference surface ``corrupt / encode / decode / denoise``.

On a CPU device it is plain torch (autograd, the reference's ``randn_like`` / ``rand_like`` draws, ``torch.optim.Adam``).
On a GPU device it rides the HIP engine like the MLP VAE: one flat parameter buffer, the four layers on the dense kernels
of csrc/dense.hip (bias and ReLU in the epilogue, the derivative read from the saved output), the corruption, tanh + squared
error and the loss on csrc/dae.hip, ``training_step`` one autograd.Function over those launches, ``FusedAdam`` and the
graph-replayed ``ModuleFastStep``.  The draw happens inside the step, so a captured graph includes it:
Gaussian noise from torch's device generator; the mask modes from Philox words under a 64-bit key that is refilled in place
from that generator every step.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from lgm_hip import ops
from lgm_hip.flat import FlatParams, _r4
from lgm_hip.lightning import LightningModule, multi_rank
from lgm_hip.nn import GradCtx, Linear, param_kind
from lgm_hip.optim import FusedAdam

HIDDEN, CODE = 256, 128
NOISE_TYPES = ("gaussian", "salt_and_pepper", "masking")


def _no_tape(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


class Encoder(nn.Module):
    """reference dae.py:12-31"""

    def __init__(self, img_channels: int = 1, img_size: int = 28):
        super().__init__()
        self.model = nn.Sequential(Linear(img_channels * img_size * img_size, HIDDEN), nn.ReLU(), Linear(HIDDEN, CODE),
                                   nn.ReLU())

    def forward(self, x):
        return self.model(x.view(x.size(0), -1))

    # ---- HIP engine: x2 [B, >= D] ------------------------------------------------------------------------------------------
    def fwd(self, x2):
        """-> the activations [x2, h1, h]; Linear -> ReLU is one launch"""
        acts = [x2]
        for i in (0, 2):
            acts.append(self.model[i].fwd(acts[-1], ops.ACT_RELU))
        return acts

    def bwd(self, gc: GradCtx, acts, g):
        g = self.model[2].bwd(gc, acts[1], acts[2], g, ops.ACT_RELU)
        self.model[0].bwd(gc, acts[0], acts[1], g, ops.ACT_RELU, need_gx=False)     # nothing upstream of the corrupted batch


class Decoder(nn.Module):
    """reference dae.py:34-51"""

    def __init__(self, img_channels: int = 1, img_size: int = 28):
        super().__init__()
        self.shape = (img_channels, img_size, img_size)
        self.model = nn.Sequential(Linear(CODE, HIDDEN), nn.ReLU(), Linear(HIDDEN, img_channels * img_size * img_size),
                                   nn.Tanh())

    def forward(self, h):
        return self.model(h).view(h.size(0), *self.shape)

    # ---- HIP engine -----------------------------------------------------------------------------------------------------
    def fwd(self, h, last_act=ops.ACT_NONE):
        """h [B, >= 128] -> the last layer's output [B, r4(D)] (before the Tanh unless last_act says otherwise), [h, h3]"""
        acts = [h, self.model[0].fwd(h, ops.ACT_RELU)]
        return self.model[2].fwd(acts[1], last_act), acts

    def bwd(self, gc: GradCtx, acts, gpre):
        """gpre: gradient at the last layer's output BEFORE the Tanh -> the gradient at h"""
        g = self.model[2].bwd(gc, acts[1], None, gpre)
        return self.model[0].bwd(gc, acts[0], acts[1], g, ops.ACT_RELU)


class DAE(LightningModule):
    def __init__(self, img_channels: int = 1, img_size: int = 28, noise_type: str = "gaussian", noise_level: float = 0.1,
                 lr: float = 1e-3, b1: float = 0.9, b2: float = 0.999, weight_decay: float = 0.0):
        super().__init__()
        if noise_type not in NOISE_TYPES:
            raise ValueError(f"Invalid noise type specified: {noise_type!r} (one of {', '.join(NOISE_TYPES)})")
        if not noise_level >= 0:
            raise ValueError(f"noise_level must be >= 0, got {noise_level}")
        self.save_hyperparameters()
        self.encoder = Encoder(img_channels, img_size)
        self.decoder = Decoder(img_channels, img_size)
        self.metric = nn.MSELoss()
        self.noise_type, self.noise_level = noise_type, noise_level
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

    # ---- corruption -----------------------------------------------------------------------------------------------------
    @property
    def dim(self) -> int:
        hp = self.hparams
        return hp.img_channels * hp.img_size * hp.img_size

    def _check_x(self, x: torch.Tensor):
        if x.dim() != 4 or tuple(x.shape[1:]) != self.decoder.shape:
            raise ValueError(f"x must be [n, {', '.join(map(str, self.decoder.shape))}], got {tuple(x.shape)}")

    def draw_key(self, device) -> torch.Tensor:
        """The step's 64-bit Philox key: ONE persistent int64 [1] device tensor, refilled in place from torch's device
        generator (one launch; capturable), as ``GaussianDiffusion.draw_dropout_key`` does it."""
        key = self.__dict__.get("mask_key")
        if key is None or key.device != torch.device(device):
            key = self.__dict__["mask_key"] = torch.zeros(1, dtype=torch.int64, device=device)
        return key.random_(-2 ** 63, None)             # all 64 bits

    def _corrupt_hip(self, x2, noise=None, key=None):
        """x2 [B, D] -> the corrupted batch [B, r4(D)] (pad lanes 0); draws what it is not given"""
        B, D = x2.shape
        out = ops.new((B, _r4(D)), x2)
        if self.noise_type == "gaussian":
            if key is not None:
                raise ValueError("gaussian corruption takes `noise`, not `key`")
            noise = torch.randn([B, D], device=x2.device) if noise is None else _no_tape(noise).reshape(B, -1)
            if tuple(noise.shape) != (B, D):
                raise ValueError(f"noise must hold {B} x {D} values, got {tuple(noise.shape)}")
            return ops.dae_corrupt(x2, noise, float(self.noise_level), out)
        if self.noise_type not in ops.DAE_MASK_MODES:
            raise ValueError("Invalid noise type specified")
        if noise is not None:
            raise ValueError(f"{self.noise_type} corruption on a GPU draws from a Philox `key`, not from `noise`")
        if key is None:
            key = self.draw_key(x2.device)
        elif not torch.is_tensor(key):
            key = torch.tensor([((int(key) + 2 ** 63) % 2 ** 64) - 2 ** 63], dtype=torch.int64, device=x2.device)
        return ops.dae_corrupt_mask(x2, key, self.noise_type, float(self.noise_level), out)

    def add_noise(self, x: torch.Tensor, noise=None) -> torch.Tensor:
        """The reference's corruption in plain torch (dae.py:167-206), with its draws; ``noise`` replaces them: the normal
        draw (gaussian), the two uniform draws stacked salt first (salt_and_pepper), the uniform draw (masking)"""
        lvl = self.noise_level
        if self.noise_type == "gaussian":
            n = torch.randn_like(x) if noise is None else noise.reshape(x.shape)
            return x + n * lvl
        if self.noise_type == "salt_and_pepper":
            if noise is None:
                salt = torch.rand_like(x)
                pepper = torch.rand_like(x)
            else:
                salt, pepper = noise[0].reshape(x.shape), noise[1].reshape(x.shape)
            x = torch.where(salt < (lvl / 2), torch.ones_like(x), x)
            return torch.where(pepper < (lvl / 2), torch.zeros_like(x), x)       # pepper wins, and pepper is 0
        if self.noise_type == "masking":
            u = torch.rand_like(x) if noise is None else noise.reshape(x.shape)
            return torch.where(u < lvl, torch.zeros_like(x), x)
        raise ValueError("Invalid noise type specified")

    # ---- engine ---------------------------------------------------------------------------------------------------------
    def run(self, x: torch.Tensor, xc: torch.Tensor, save: bool):
        """x [B, C, S, S] the clean batch, xc [B, >= D] its corrupted rows -> (vals [1] = (loss,), x_hat [B, r4(D)]), tape"""
        D, B = self.dim, x.shape[0]
        x2 = x.view(B, D)
        enc = self.encoder.fwd(xc)
        pre, dec = self.decoder.fwd(enc[2])
        xh = ops.new(pre.shape, pre)
        rpart = ops.new((B,), pre)
        ops.dae_tanh_mse_fwd(pre, x2, D, xh, rpart)
        vals = ops.new((1,), pre)
        ops.dae_loss(rpart, D, vals)
        return (vals, xh), ((x2, enc, dec, xh) if save else None)

    def backward_hip(self, tape, gloss):
        """gloss: device scalar d L / d loss; writes the flat gradient buffer"""
        x2, enc, dec, xh = tape
        gc = GradCtx(self._flat)                 # refreshes the transposed weight copies the input gradients read
        gpre = ops.new(xh.shape, xh)
        ops.dae_tanh_mse_bwd(xh, x2, gloss, self.dim, gpre)
        self.encoder.bwd(gc, enc, self.decoder.bwd(gc, dec, gpre))
        gc.flush()
        self._flat.bind_grad_views()

    def _image(self, xh: torch.Tensor) -> torch.Tensor:
        return xh[:, :self.dim].reshape(-1, *self.decoder.shape)

    # ---- the reference's surface ----------------------------------------------------------------------------------------
    def forward(self, x):
        if x.device.type == "cuda":
            return self.denoise(x)
        return self.decoder(self.encoder(x))

    def _common_step(self, batch, batch_idx, corrupted=None):
        x, _ = batch
        self._check_x(x)
        if self._on_hip(x):
            return _DAEStepFn.apply(self._anchor(x.device), self, x, corrupted)
        noisy = self.add_noise(x) if corrupted is None else corrupted
        return self.metric(x, self.decoder(self.encoder(noisy)))

    def training_step(self, batch, batch_idx, corrupted=None):
        """``corrupted`` [B, C, S, S]: an already corrupted batch that replaces the draw (nothing is drawn)"""
        loss = self._common_step(batch, batch_idx, corrupted)
        self.log("loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        return loss

    def validation_step(self, batch, batch_idx, corrupted=None):
        if batch[0].device.type == "cuda":
            with torch.no_grad():                # the same forward, no tape
                loss = self._common_step(batch, batch_idx, corrupted)
        else:
            loss = self._common_step(batch, batch_idx, corrupted)
        self.log("val_loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        return loss

    def configure_optimizers(self):
        hp = self.hparams
        if self._flat is not None:
            return FusedAdam(self.parameters(), lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)
        return torch.optim.Adam(self.parameters(), lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)

    def make_fast_step(self, opt, world: int = 1, use_graph: bool = True, accumulate: int = 1):
        """The step object ``MiniTrainer.fit`` drives: training_step + backward replayed from one HIP graph (the draw of the
        corruption included), eager fallback inside."""
        from lgm_hip.graph import ModuleFastStep
        self.prepare_hip(next(self.parameters()).device)
        if self._flat is None:
            raise RuntimeError("make_fast_step needs the model on a GPU device")
        return ModuleFastStep(self, opt, world, use_graph, accumulate=accumulate)

    # ---- inference: both devices; launch sequences without a tape on the GPU ----------------------------------------------
    @torch.no_grad()
    def corrupt(self, x: torch.Tensor, noise=None, key=None):
        """x [B, C, S, S] -> its corrupted copy.  ``noise``: the draws of the plain-torch formula (see ``add_noise``; on a GPU
        the gaussian mode alone takes them).  ``key``: the 64-bit Philox key of the mask modes on a GPU (an int, or an int64
        [1] device tensor).  What is not given is drawn."""
        self._check_x(x)
        if not self._on_hip(x):
            if key is not None:
                raise ValueError("a Philox `key` applies on a GPU device; on the CPU pass the draws as `noise`")
            return self.add_noise(x, noise)
        x = _no_tape(x)
        return self._image(self._corrupt_hip(x.view(x.shape[0], -1), noise, key))

    @torch.no_grad()
    def encode(self, x: torch.Tensor):
        """x [B, C, S, S] -> the code [B, 128]"""
        self._check_x(x)
        if not self._on_hip(x):
            return self.encoder(x)
        x = _no_tape(x)
        return self.encoder.fwd(x.view(x.shape[0], -1))[2]

    def _check_h(self, h: torch.Tensor):
        if h.dim() != 2 or h.shape[1] != CODE:
            raise ValueError(f"h must be [n, {CODE}], got {tuple(h.shape)}")

    @torch.no_grad()
    def decode(self, h: torch.Tensor):
        """h [n, 128] -> images [n, C, S, S] in (-1, 1)"""
        self._check_h(h)
        if not self._on_hip(h):
            return self.decoder(h)
        xh, _ = self.decoder.fwd(_no_tape(h), ops.ACT_TANH)
        return self._image(xh)

    @torch.no_grad()
    def denoise(self, x: torch.Tensor):
        """decode(encode(x)): the reconstruction of a (noisy) batch, nothing is corrupted here"""
        return self.decode(self.encode(x))


class _DAEStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, m: DAE, x, corrupted):
        ctx.set_materialize_grads(False)
        save = bool(ctx.needs_input_grad[0])
        x = _no_tape(x)
        B = x.shape[0]
        if corrupted is None:
            xc = m._corrupt_hip(x.view(B, -1))       # drawn from the device generator, inside the step: captured with it
        else:
            xc = _no_tape(corrupted).view(B, -1)
        (vals, _), tape = m.run(x, xc, save)
        ctx.stuff = (m, tape)
        return vals[0]

    @staticmethod
    def backward(ctx, gloss):
        m, tape = ctx.stuff
        if tape is None:
            raise RuntimeError("DAE step ran without saving activations")
        m.backward_hip(tape, gloss.detach().float().reshape(1).contiguous())
        ctx.stuff = None
        return None, None, None, None
