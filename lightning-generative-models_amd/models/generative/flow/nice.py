"""NICE (Dinh et al. 2015) - drop-in for the reference's models/generative/flow/nice.py: same class names, state_dict keys
(``layers.{i}.transformation.net.{0,2}``, ``scaling_layer.log_scale`` last), parameter order, default arithmetic, logged name
(``train_loss``) and optimiser (Adam, lr 1e-3).  The reference is unfinished, and what finishes it sits behind keywords that
default to its behaviour:

``alternate``     the reference shifts lanes [D/2, D) by a function of lanes [0, D/2) in EVERY layer, so the first half is never
                  transformed; ``alternate=True`` swaps the two roles on odd layers (same keys and shapes).
``exact_logdet``  the reference's loss is -(mean_ll - sum log_scale): it subtracts the log-determinant where the change of
                  variables adds it, and is unbounded below as log_scale -> -inf.  ``exact_logdet=True`` is the negative mean
                  log-likelihood -(mean_ll + sum log_scale).
Also beyond the reference: ``hidden_dim`` and the optimiser's hyperparameters, image batches [B, C, S, S] (flattened as a view),
``validation_step``, and the inference surface ``log_prob / inverse / sample``.

On a CPU device it is plain torch.  On a GPU device it rides the HIP engine like the DAE: one flat parameter buffer, the
coupling nets on the dense kernels of csrc/dense.hip (bias and LeakyReLU in the epilogue), the coupling, the scaling layer,
its backward and the loss on csrc/nice.hip, ``training_step`` one autograd.Function over those launches, ``FusedAdam`` and the
graph-replayed ``ModuleFastStep``.  No half is ever chunked, concatenated or copied: a coupling net reads
its conditioning half as a pitched view of the state buffer, and its backward reads the shifted half's gradient the same way.
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
LOG_2PI = math.log(2.0 * math.pi)


def _no_tape(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


class CouplingNet(nn.Module):
    """reference nice.py:7-19"""

    def __init__(self, in_dim: int, hidden_dim: int):
        super().__init__()
        self.net = nn.Sequential(Linear(in_dim, hidden_dim), nn.LeakyReLU(SLOPE), Linear(hidden_dim, in_dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.net(x)

    # ---- HIP engine: xc [B, in_dim] is a lane slice of a state buffer ----------------------------------------------------------
    def fwd(self, xc):
        """-> (t [B, r4(in_dim)], the hidden activation): Linear -> LeakyReLU is one launch"""
        a = self.net[0].fwd(xc, ops.ACT_LRELU, SLOPE, x_sliced=True)
        return self.net[2].fwd(a), a

    def bwd(self, gc: GradCtx, xc, a, gt):
        """gt [B, in_dim]: a lane slice of the gradient buffer -> the gradient at xc [B, r4(in_dim)]"""
        ga = self.net[2].bwd(gc, a, None, gt, gy_sliced=True)
        return self.net[0].bwd(gc, xc, a, ga, ops.ACT_LRELU, SLOPE, x_sliced=True)


class CouplingLayer(nn.Module):
    """reference nice.py:22-33; ``swap``: lanes [0, D/2) are shifted by a function of lanes [D/2, D)"""

    def __init__(self, dim: int, hidden_dim: int = 256, swap: bool = False):
        super().__init__()
        self.half, self.swap = dim // 2, bool(swap)
        self.transformation = CouplingNet(dim // 2, hidden_dim)

    @property
    def cond_off(self) -> int:
        return self.half if self.swap else 0

    @property
    def shift_off(self) -> int:
        return 0 if self.swap else self.half

    def forward(self, x: torch.Tensor, reverse: bool = False) -> torch.Tensor:
        """Plain torch: the shifted half is ``s + net(c)`` (``s - net(c)`` in reverse), the conditioning half passes through"""
        c, s = self.cond(x), x[:, self.shift_off:self.shift_off + self.half]
        t = self.transformation(c)
        y = s - t if reverse else s + t
        return torch.cat([y, c] if self.swap else [c, y], dim=1)

    # ---- HIP engine: s [B, >= D] the state ------------------------------------------------------------------------------------
    def cond(self, s):
        return s[:, self.cond_off:self.cond_off + self.half]

    def fwd(self, s, sign: int = 1, out=None):
        """-> (the next state [B, r4(D)], the hidden activation); ``out`` may be ``s`` itself (no tape is kept then)"""
        t, a = self.transformation.fwd(self.cond(s))
        out = ops.new((s.shape[0], _r4(2 * self.half)), s) if out is None else out
        return ops.nice_couple(s[:, :2 * self.half], t[:, :self.half], self.shift_off, sign, out), a

    def bwd(self, gc: GradCtx, s, a, g):
        """g [B, r4(D)]: the gradient at this layer's output, turned into the gradient at its input in place"""
        gt = g[:, self.shift_off:self.shift_off + self.half]
        gx = self.transformation.bwd(gc, self.cond(s), a, gt)
        ops.nice_couple(g[:, :2 * self.half], gx[:, :self.half], self.cond_off, 1, g)


class ScalingLayer(nn.Module):
    """reference nice.py:36-46"""

    def __init__(self, dim: int):
        super().__init__()
        self.log_scale = nn.Parameter(torch.zeros(dim))

    def forward(self, x: torch.Tensor, reverse: bool = False) -> torch.Tensor:
        return x * torch.exp(-self.log_scale if reverse else self.log_scale)


class NICE(LightningModule):
    def __init__(self, input_dim: Optional[int] = None, n_coupling_layers: int = 4, hidden_dim: int = 256,
                 img_channels: Optional[int] = None, img_size: Optional[int] = None, lr: float = 1e-3, b1: float = 0.9,
                 b2: float = 0.999, weight_decay: float = 0.0, alternate: bool = False, exact_logdet: bool = False):
        super().__init__()
        shape = None
        if img_channels is not None or img_size is not None:
            if img_channels is None or img_size is None:
                raise ValueError("img_channels and img_size go together")
            shape = (int(img_channels), int(img_size), int(img_size))
            d_img = shape[0] * shape[1] * shape[2]
            if input_dim is not None and int(input_dim) != d_img:
                raise ValueError(f"input_dim {input_dim} contradicts img_channels * img_size^2 = {d_img}")
            input_dim = d_img
        if input_dim is None:
            raise ValueError("input_dim (or img_channels and img_size) is required")
        input_dim = int(input_dim)
        if input_dim < 2 or input_dim % 2:
            raise ValueError(f"input_dim must be positive and even, got {input_dim}")
        if n_coupling_layers < 1:
            raise ValueError(f"n_coupling_layers must be >= 1, got {n_coupling_layers}")
        if hidden_dim < 1:
            raise ValueError(f"hidden_dim must be >= 1, got {hidden_dim}")
        self.save_hyperparameters()
        self.dim, self.img_shape = input_dim, shape
        self.alternate, self.exact_logdet = bool(alternate), bool(exact_logdet)
        self.layers = nn.ModuleList([CouplingLayer(input_dim, hidden_dim, swap=self.alternate and i % 2 == 1)
                                     for i in range(n_coupling_layers)])
        self.scaling_layer = ScalingLayer(input_dim)
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

    # ---- shapes ---------------------------------------------------------------------------------------------------------
    def _rows(self, x: torch.Tensor, what: str = "x") -> torch.Tensor:
        """[B, D] or [B, C, S, S] -> the [B, D] view"""
        if x.dim() == 4 and (self.img_shape is None or tuple(x.shape[1:]) == self.img_shape):
            x = x.reshape(x.shape[0], -1)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"{what} must hold rows of {self.dim} values, got {tuple(x.shape)}")
        return x

    # ---- engine ---------------------------------------------------------------------------------------------------------
    def _ls(self) -> int:
        return self._flat.ptr(self.scaling_layer.log_scale)

    def run(self, x2: torch.Tensor, save: bool):
        """x2 [B, D] -> (vals3 = (loss, mean_ll, sum log_scale), z [B, r4(D)], row_part [B]), tape"""
        D, B = self.dim, x2.shape[0]
        states, hidden = [x2], []
        for i, layer in enumerate(self.layers):
            # without a tape every layer after the first overwrites the state it reads (the first leaves the batch alone)
            s, a = layer.fwd(states[-1], 1, None if save or i == 0 else states[-1])
            states.append(s)
            hidden.append(a)
        z = ops.new((B, _r4(D)), x2)
        rpart = ops.new((B,), x2)
        ops.nice_scale_fwd(states[-1], self._ls(), D, False, z, rpart)
        vals = ops.new((3,), x2)
        ops.nice_loss(rpart, self._ls(), D, self.exact_logdet, vals)
        return (vals, z, rpart), ((states, hidden, z) if save else None)

    def backward_hip(self, tape, gloss):
        """gloss: device scalar d L / d loss; writes the flat gradient buffer"""
        states, hidden, z = tape
        gc = GradCtx(self._flat)                 # refreshes the transposed weight copies the input gradients read
        ls = self.scaling_layer.log_scale
        g = ops.new(z.shape, z)
        ops.nice_scale_bwd(z, self._ls(), gloss, self.dim, self.exact_logdet, g, self._flat.gptr(ls), gc.beta(ls))
        for i in range(len(self.layers) - 1, -1, -1):
            self.layers[i].bwd(gc, states[i], hidden[i], g)
        gc.flush()
        self._flat.bind_grad_views()

    def _inverse_hip(self, z2: torch.Tensor) -> torch.Tensor:
        D = self.dim
        s = ops.new((z2.shape[0], _r4(D)), z2)
        ops.nice_scale_fwd(z2, self._ls(), D, True, s, None)
        for layer in reversed(self.layers):
            layer.fwd(s, -1, s)
        return s[:, :D]

    # ---- the reference's surface ----------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, reverse: bool = False) -> torch.Tensor:
        shape = x.shape
        x2 = self._rows(x, "z" if reverse else "x")
        if self._on_hip(x2):
            with torch.no_grad():
                x2 = _no_tape(x2)
                out = self._inverse_hip(x2) if reverse else self.run(x2, False)[0][1][:, :self.dim]
            return out.reshape(shape)
        if reverse:
            x2 = self.scaling_layer(x2, reverse)
            for layer in reversed(self.layers):
                x2 = layer(x2, reverse)
        else:
            for layer in self.layers:
                x2 = layer(x2)
            x2 = self.scaling_layer(x2)
        return x2.reshape(shape)

    def _compute_loss(self, z: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """reference nice.py:68-73 (the caller negates it); ``exact_logdet`` turns the sign of the log-determinant"""
        z = z.reshape(z.shape[0], -1)
        # the constant as the reference forms it: from a float32 tensor, whatever z's dtype
        const = 0.5 * z.size(1) * torch.log(2 * torch.tensor(torch.pi))
        ll = -0.5 * z.pow(2).sum(1) - const
        logdet = self.scaling_layer.log_scale.sum()
        return ((ll + logdet) if self.exact_logdet else (ll - logdet)).mean()

    def _common_step(self, batch, batch_idx):
        x, _ = batch
        x2 = self._rows(x)
        if self._on_hip(x2):
            return _NICEStepFn.apply(self._anchor(x2.device), self, x2)
        return -self._compute_loss(self(x2), x2)

    def training_step(self, batch, batch_idx):
        loss = self._common_step(batch, batch_idx)
        self.log("train_loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        return loss

    def validation_step(self, batch, batch_idx):
        with torch.no_grad():                    # the same forward, no tape
            loss = self._common_step(batch, batch_idx)
        self.log("val_loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        return loss

    def configure_optimizers(self):
        hp = self.hparams
        if self._flat is not None:
            return FusedAdam(self.parameters(), lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)
        return torch.optim.Adam(self.parameters(), lr=hp.lr, betas=(hp.b1, hp.b2), weight_decay=hp.weight_decay)

    def make_fast_step(self, opt, world: int = 1, use_graph: bool = True, accumulate: int = 1):
        """The step object ``MiniTrainer.fit`` drives: training_step + backward replayed from one HIP graph, eager fallback
        inside."""
        from lgm_hip.graph import ModuleFastStep
        self.prepare_hip(next(self.parameters()).device)
        if self._flat is None:
            raise RuntimeError("make_fast_step needs the model on a GPU device")
        return ModuleFastStep(self, opt, world, use_graph, accumulate=accumulate)

    # ---- inference: both devices; launch sequences without a tape on the GPU ----------------------------------------------
    @torch.no_grad()
    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, D] or [B, C, S, S] -> log p(x) [B], the exact density whatever ``exact_logdet`` says:
        -0.5 sum z^2 - 0.5 D log 2 pi + sum log_scale"""
        x2 = self._rows(x)
        if self._on_hip(x2):
            (vals, _, rpart), _ = self.run(_no_tape(x2), False)
            return rpart * -0.5 + (vals[2] - 0.5 * self.dim * LOG_2PI)      # [B] values from the kernels' sums
        z = self(x2)
        return -0.5 * z.pow(2).sum(1) - 0.5 * self.dim * LOG_2PI + self.scaling_layer.log_scale.sum()

    @torch.no_grad()
    def inverse(self, z: torch.Tensor) -> torch.Tensor:
        """z [n, D] (or an image-shaped batch) -> x of the same shape: ``forward(z, reverse=True)``"""
        return self(z, reverse=True)

    @torch.no_grad()
    def sample(self, n: int, z: Optional[torch.Tensor] = None, temperature: float = 1.0) -> torch.Tensor:
        """n draws z ~ N(0, temperature^2 I) (or the given ``z`` [n, D]) through the inverse -> [n, C, S, S] when the image
        shape is known, [n, D] otherwise"""
        if not temperature > 0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if z is None:
            p = self.scaling_layer.log_scale
            z = torch.randn(int(n), self.dim, device=p.device, dtype=p.dtype) * temperature
        elif z.dim() != 2 or tuple(z.shape) != (int(n), self.dim):
            raise ValueError(f"z must be [{int(n)}, {self.dim}], got {tuple(z.shape)}")
        x = self.inverse(z)
        return x.reshape(-1, *self.img_shape) if self.img_shape is not None else x


class _NICEStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, m: NICE, x2):
        ctx.set_materialize_grads(False)
        save = bool(ctx.needs_input_grad[0])
        (vals, _, _), tape = m.run(_no_tape(x2), save)
        ctx.stuff = (m, tape)
        return vals[0]

    @staticmethod
    def backward(ctx, gloss):
        m, tape = ctx.stuff
        if tape is None:
            raise RuntimeError("NICE step ran without saving activations")
        m.backward_hip(tape, gloss.detach().float().reshape(1).contiguous())
        ctx.stuff = None
        return None, None, None
