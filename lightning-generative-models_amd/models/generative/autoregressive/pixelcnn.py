"""Gated PixelCNN on the MI355X HIP engine - the reference's models/generative/autoregressive/pixelcnn.py (``MaskedConv2d``,
``GatedBlock``, ``PixelCNN``: same class names, constructor arguments, state_dict keys, shapes and parameter order, the
``mask`` buffers included), finished: a prior over the VQ-VAE's codes that trains on the graph-replayed step and samples
incrementally.

Masked convolutions run on lgm_mconv_* (csrc/pixelcnn.hip): the live taps of a type-A / type-B mask are a prefix of the tap
axis of the physical weight [Nw][k*k][Cw], the kernels stop at the last live tap and never read a dead one (the backward's
default route is the generic pair on the zero-masked weights, where that measured faster: ``MaskedConv2d.backward_route``).  Dead taps are
zeroed at construction and after ``load_state_dict`` and their gradient is zero, so Adam leaves them at zero (the reference
gives them a gradient that its next forward masks away: parity is defined on the live taps).  Forward and backward are
explicit launch sequences; autograd sees one Function.

``sample`` walks the grid once: per position one incremental step of every layer (lgm_pixelcnn_step reads the cached
activations of the earlier positions, Ramachandran et al. 2017) and one draw (lgm_categorical_draw), captured once and replayed
``h * w`` times - not ``h * w`` full forwards.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch import nn

from lgm_hip import ops
from lgm_hip.captured import _CapturedStep, _cached_step
from lgm_hip.flat import FlatParams, _r4
from lgm_hip.lightning import LightningModule, multi_rank
from lgm_hip.nn import Conv2d, GradCtx, _flat, param_kind
from lgm_hip.optim import FusedAdam


def live_taps(kernel_size: int, mask_type: str) -> int:
    """Taps a type-A / type-B mask keeps: those whose row-major index kh * k + kw is below this count."""
    k = kernel_size
    return (k // 2) * k + k // 2 + (1 if mask_type == "B" else 0)


class MaskedConv2d(Conv2d):
    """reference pixelcnn.py:8-23: ``MaskedConv2d(mask_type, in_channels, out_channels, kernel_size, stride, padding)``."""

    # Which kernels the two gradients run on.  Measured at the prior's working shapes (B = 256, 8 x 8 codes, 64 -> 128 and
    # 128 -> 256, k = 7; profiles/r22_pixelcnn_bench.json): the live-tap forward is 0.77 - 0.83 of lgm_conv_xy's time on the
    # zero-masked weights and stays; the live-tap input gradient (1.41 - 1.68) and weight gradient (2.4 - 5.9) are slower than
    # lgm_conv_yx / lgm_conv_wgrad computing all 49 taps, so the backward takes the generic kernels on the zero-masked weights
    # and lgm_mconv_zero_dead restores the dead taps' zero gradient.  "masked": lgm_mconv_yx / lgm_mconv_wgrad.
    backward_route = "generic"

    def __init__(self, mask_type: str, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1,
                 padding: int = 0, bias: bool = True):
        if mask_type not in ("A", "B"):
            raise ValueError(f"mask_type must be 'A' or 'B', got {mask_type!r}")
        if kernel_size % 2 == 0:
            raise ValueError(f"a masked convolution needs an odd kernel size, got {kernel_size}")
        if stride != 1 or padding != kernel_size // 2:
            raise ValueError(f"a masked convolution keeps the map: stride 1 and padding {kernel_size // 2} expected, "
                             f"got stride {stride}, padding {padding}")
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias)
        self.mask_type = mask_type
        self.taps_live = live_taps(kernel_size, mask_type)
        mask = torch.ones_like(self.weight.data)
        mask[:, :, kernel_size // 2, kernel_size // 2 + (mask_type == "B"):] = 0
        mask[:, :, kernel_size // 2 + 1:] = 0
        self.register_buffer("mask", mask)
        self.zero_dead_taps()

    @torch.no_grad()
    def zero_dead_taps(self):
        self.weight.data.mul_(self.mask.to(self.weight.device))

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.zero_dead_taps()

    def fwd(self, x):
        B, H, W, C = x.shape
        assert C == _r4(self.cin), f"conv expects {_r4(self.cin)} (padded) channels, got {C}"
        g = self.geom(B, H, W)
        fp = _flat(self.weight)
        y = ops.new((B, H, W, _r4(self.cout)), x)
        ops.lib().lgm_mconv_xy(ctypes.byref(g), self.taps_live, x.data_ptr(), ops.pitch(x), fp.ptr(self.weight),
                               fp.ptr(self.bias) if self.bias is not None else None, y.data_ptr(), ops.pitch(y), ops.stream())
        return y

    def bwd(self, gc: GradCtx, x, gy, need_gx=True, res=None):
        """gW (dead taps zero), gb into the flat gradients; returns gx = dgrad(gy) (+ res)."""
        B, H, W, _ = x.shape
        g = self.geom(B, H, W)
        fp = gc.flat
        L = ops.lib()
        bw = gc.beta(self.weight)
        gb = None
        if self.bias is not None:
            bb = gc.beta(self.bias)
            if bb == bw:
                gb = fp.gptr(self.bias)
            else:
                ops.colsum(gy, fp.gptr(self.bias), bb)
        if self.backward_route == "generic":
            ops.conv_wgrad(g, gy, x, fp.gptr(self.weight), bw, gb)
            L.lgm_mconv_zero_dead(ctypes.byref(g), self.taps_live, fp.gptr(self.weight), ops.stream())
            if not need_gx:
                return None
            gx = ops.new(x.shape, x)
            ops.conv_yx(g, gy, fp.ptr(self.weight), None, res, gx, fp.tptr(self.weight))
            return gx
        nbytes = L.lgm_mconv_wgrad_workspace(ctypes.byref(g), self.taps_live)
        ws = ops.workspace(nbytes, x.device)
        L.lgm_mconv_wgrad(ctypes.byref(g), self.taps_live, gy.data_ptr(), ops.pitch(gy), x.data_ptr(), ops.pitch(x),
                          fp.gptr(self.weight), gb, bw, ws.data_ptr(), ws.numel() * 4, ops.stream())
        if not need_gx:
            return None
        gx = ops.new(x.shape, x)
        L.lgm_mconv_yx(ctypes.byref(g), self.taps_live, gy.data_ptr(), ops.pitch(gy), fp.ptr(self.weight),
                       None if res is None else res.data_ptr(), 0 if res is None else ops.pitch(res), gx.data_ptr(),
                       ops.pitch(gx), ops.stream())
        return gx


class GatedBlock(nn.Module):
    """reference pixelcnn.py:26-45: x (-> skip) + tanh(a) sigmoid(b), (a, b) = chunk(MaskedConv2d_B(x), 2)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        if out_channels % 4:
            raise ValueError(f"the gate's halves are read 16 bytes at a time: out_channels % 4 == 0 expected, got {out_channels}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv = MaskedConv2d("B", in_channels, 2 * out_channels, 7, 1, 3)
        self.skip = Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None

    def fwd(self, x):
        pre = self.conv.fwd(x)
        xs = self.skip.fwd(x) if self.skip is not None else x
        B, H, W, _ = x.shape
        y = ops.new((B, H, W, self.out_channels), x)
        ops.lib().lgm_gated_fwd(xs.data_ptr(), ops.pitch(xs), pre.data_ptr(), ops.pitch(pre), B * H * W, self.out_channels,
                                y.data_ptr(), ops.pitch(y), ops.stream())
        return y, (x, pre)

    def bwd(self, gc: GradCtx, saved, gy):
        x, pre = saved
        B, H, W, _ = x.shape
        # (ga, gb) over the saved pre-activation; the residual's gradient rides in the input gradient's epilogue
        ops.lib().lgm_gated_bwd(gy.data_ptr(), ops.pitch(gy), pre.data_ptr(), ops.pitch(pre), B * H * W, self.out_channels,
                                None, 0, pre.data_ptr(), ops.pitch(pre), ops.stream())
        res = self.skip.bwd(gc, x, gy) if self.skip is not None else gy
        return self.conv.bwd(gc, x, pre, res=res)


class PixelCNN(LightningModule):
    """reference pixelcnn.py:48-106 plus ``img_size`` / ``img_channels`` (the loader's cross-check; without a VQ-VAE ``img_size``
    is also the side of the sampled grid), ``vqvae`` ({"args": {...}, "ckpt_path": ...} or a ``VQVAE``: the frozen model whose
    codes this prior models - its quantised latents are the input, its indices the targets) and ``temperature``."""

    def __init__(self, input_channels: int, hidden_channels: int, output_channels: int, num_layers: int = 5,
                 learning_rate: float = 1e-3, img_size: Optional[int] = None, img_channels: Optional[int] = None,
                 vqvae=None, temperature: float = 1.0) -> None:
        super().__init__()
        self.save_hyperparameters()
        if not isinstance(vqvae, dict):
            self._hparams["vqvae"] = None            # an instance is no hyper-parameter: checkpoints carry it under vqvae.*
        if temperature <= 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        self.learning_rate = learning_rate
        self.input_channels, self.hidden_channels, self.output_channels = input_channels, hidden_channels, output_channels
        self.img_size, self.img_channels, self.temperature = img_size, img_channels, float(temperature)
        self.input_conv = MaskedConv2d("A", input_channels, hidden_channels, 7, 1, 3)
        self.gated_blocks = nn.ModuleList([GatedBlock(hidden_channels, hidden_channels) for _ in range(num_layers)])
        self.output_conv = Conv2d(hidden_channels, output_channels, 1)
        self._flat: Optional[FlatParams] = None
        self.__dict__["_vqvae"] = self._make_vqvae(vqvae)        # not a submodule: no parameter of the prior
        if self._vqvae is not None:
            hp = self._vqvae.hparams
            if input_channels != hp.embedding_dim:
                raise ValueError(f"input_channels {input_channels} != the VQ-VAE's embedding_dim {hp.embedding_dim}")
            if output_channels != hp.num_embeddings:
                raise ValueError(f"output_channels {output_channels} != the VQ-VAE's num_embeddings {hp.num_embeddings}")
            self.grid = (hp.img_size // 8, hp.img_size // 8)
        else:
            self.grid = (img_size, img_size) if img_size is not None else None

    # ---- the frozen VQ-VAE ------------------------------------------------------------------------------------------------
    @staticmethod
    def _make_vqvae(spec):
        if spec is None:
            return None
        from models.generative.vae.vqvae import VQVAE
        if isinstance(spec, VQVAE):
            model = spec
        elif isinstance(spec, dict) and "args" in spec:
            model = VQVAE(**spec["args"])
            if spec.get("ckpt_path"):
                ckpt = torch.load(spec["ckpt_path"], map_location="cpu", weights_only=False)
                model.load_state_dict(ckpt.get("state_dict", ckpt))
        else:
            raise ValueError("vqvae must be a VQVAE or {'args': {...}, 'ckpt_path': ...}")
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
        return model

    @property
    def vqvae(self):
        return self._vqvae

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self._vqvae is not None:
            self._vqvae._apply(fn, *args, **kwargs)
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self._vqvae is not None:
            for k, v in self._vqvae.state_dict().items():
                destination[f"{prefix}vqvae.{k}"] = v

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        tp = f"{prefix}vqvae."
        found = {k[len(tp):]: v for k, v in state_dict.items() if k.startswith(tp)}
        for k in [k for k in state_dict if k.startswith(tp)]:       # the caller's copy: nothing of it is "unexpected" later
            del state_dict[k]
        if self._vqvae is not None:
            if found:
                try:
                    self._vqvae.load_state_dict(found)
                except RuntimeError as e:
                    error_msgs.append(f"vqvae: {e}")
            else:
                missing_keys.extend(tp + k for k in self._vqvae.state_dict())
        elif found:
            unexpected_keys.extend(tp + k for k in found)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # ---- flat storage -------------------------------------------------------------------------------------------------------
    def prepare_hip(self, device) -> FlatParams:
        device = torch.device(device)
        if self._flat is not None and self._flat.device == device and self._flat.still_bound():
            return self._flat
        named = [(n, p, param_kind(n, p)) for n, p in self.named_parameters()]
        self._flat = FlatParams(named, device)
        return self._flat

    def refresh_derived_weights(self, *args, **kwargs):
        """The masked kernels read the weights themselves: nothing is derived from them."""

    def _anchor(self, device):
        self.prepare_hip(device)
        a = getattr(self, "_anchor_t", None)
        if a is None or a.device != torch.device(device):
            a = torch.zeros(1, device=device, requires_grad=True)
            self._anchor_t = a
        return a

    # ---- engine -------------------------------------------------------------------------------------------------------------
    def _nhwc(self, x: torch.Tensor) -> torch.Tensor:
        B, C, H, W = x.shape
        if C != self.input_channels:
            raise ValueError(f"expected {self.input_channels} input channels, got {C}")
        x4 = ops.new((B, H, W, _r4(C)), x)
        ops.nchw_to_nhwc(x.detach().float().contiguous(), x4)
        return x4

    def logits_nhwc(self, x4: torch.Tensor, save: bool = False):
        """x4 [B, H, W, r4(input_channels)] -> logits [B, H, W, r4(output_channels)] and the tape."""
        h = self.input_conv.fwd(x4)
        tapes = []
        for blk in self.gated_blocks:
            h, t = blk.fwd(h)
            tapes.append(t if save else None)
        return self.output_conv.fwd(h), ((x4, tapes, h) if save else None)

    def run(self, x4: torch.Tensor, target: torch.Tensor, save: bool):
        """-> (vals = (mean loss,), tape): cross-entropy of the logits at every position against ``target`` [B * H * W]."""
        logits, tape = self.logits_nhwc(x4, save)
        M, K = target.numel(), self.output_channels
        rows = ops.new((2, M), x4)                    # per-row loss and log-sum-exp
        mean = ops.new((1,), x4)
        ops.lib().lgm_softmax_xent_fwd(logits.data_ptr(), ops.pitch(logits), target.data_ptr(), M, K, rows[0].data_ptr(),
                                       rows[1].data_ptr(), mean.data_ptr(), ops.stream())
        return mean, logits, ((tape, logits, rows, target) if save else None)

    def backward_hip(self, tape, gloss):
        (x4, tapes, h_last), logits, rows, target = tape
        M, K = target.numel(), self.output_channels
        gc = GradCtx(self._flat, defer=True)
        g = ops.new(logits.shape, logits)
        ops.lib().lgm_softmax_xent_bwd(logits.data_ptr(), ops.pitch(logits), target.data_ptr(), rows[1].data_ptr(),
                                       gloss.data_ptr(), M, K, logits.shape[-1], g.data_ptr(), ops.pitch(g), ops.stream())
        g = self.output_conv.bwd(gc, h_last, g)
        for blk, t in zip(reversed(self.gated_blocks), reversed(tapes)):
            g = blk.bwd(gc, t, g)
        self.input_conv.bwd(gc, x4, g, need_gx=False)
        gc.flush()
        self._flat.bind_grad_views()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, input_channels, H, W] -> logits [B, output_channels, H, W] (inference / no-grad use)."""
        self.prepare_hip(x.device)
        B, _, H, W = x.shape
        logits, _ = self.logits_nhwc(self._nhwc(x))
        out = ops.new((B, self.output_channels, H, W), x)
        ops.nhwc_to_nchw(logits, out)
        return out

    def _batch(self, batch):
        """-> (x4 NHWC, target [M] int64): the reference's (data, target), or with a VQ-VAE the codes of the batch's images."""
        if self._vqvae is None:
            data, target = batch
            if target.dtype != torch.long or tuple(target.shape) != (data.shape[0], data.shape[2], data.shape[3]):
                raise ValueError(f"target must be int64 [B, H, W] = {(data.shape[0], data.shape[2], data.shape[3])}, "
                                 f"got {target.dtype} {tuple(target.shape)}")
            self.prepare_hip(data.device)
            return self._nhwc(data), target.reshape(-1).contiguous()
        x = batch[0]
        self.prepare_hip(x.device)
        self._vqvae.eval()
        with torch.no_grad():
            q, idx = self._vqvae.quantize(x)
        return q, idx.reshape(-1)

    def _common_step(self, batch, split: str):
        x4, target = self._batch(batch)
        loss = _PixelCNNStepFn.apply(self._anchor(x4.device), self, x4, target)
        self.log(f"{split}_loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        return loss

    def training_step(self, batch, batch_idx):
        return self._common_step(batch, "train")

    def validation_step(self, batch, batch_idx):
        return self._common_step(batch, "val")

    def configure_optimizers(self):
        return FusedAdam(self.parameters(), lr=self.learning_rate)

    def make_fast_step(self, opt, world: int = 1, use_graph: bool = True, accumulate: int = 1):
        """The step object ``MiniTrainer.fit`` drives: training_step + backward replayed from one HIP graph."""
        from lgm_hip.graph import ModuleFastStep
        self.prepare_hip(next(self.parameters()).device)
        return ModuleFastStep(self, opt, world, use_graph, accumulate=accumulate)

    # ---- sampling -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, num_samples: int, temperature: Optional[float] = None, uniforms: Optional[torch.Tensor] = None,
               return_codes: bool = False):
        """``h * w`` incremental steps, one per position in raster order.  ``uniforms`` [h * w, num_samples] in [0, 1): the
        draws' inverse-CDF arguments, else drawn on the device.  With a VQ-VAE: decoded images [B, img_channels, S, S] (and the
        codes [B, h, w] with ``return_codes``); without one the reference's result: the drawn index as a float in every channel,
        [B, input_channels, h, w]."""
        if self.grid is None:
            raise ValueError("sample() needs the grid: construct the PixelCNN with img_size or a vqvae")
        temperature = self.temperature if temperature is None else float(temperature)
        if temperature <= 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        dev = self.device
        self.prepare_hip(dev)
        h, w = self.grid
        B = int(num_samples)
        if uniforms is not None and tuple(uniforms.shape) != (h * w, B):
            raise ValueError(f"uniforms must be [{h * w}, {B}], got {tuple(uniforms.shape)}")
        cb = None if self._vqvae is None else self._vqvae.prepare_hip(dev).ptr(self._vqvae.vector_quantizer.embedding.weight)
        chain = _cached_step(self, ("pixelcnn", B, h, w, temperature, cb),
                             lambda: _PixelChain(self, B, temperature, cb, capture=True), "pixelcnn sampling", dev)
        if chain is None:
            chain = _PixelChain(self, B, temperature, cb, capture=False)
        codes, xin = chain.run(uniforms)
        if self._vqvae is not None:
            imgs = self._vqvae.decode_codes(codes)
            return (imgs, codes) if return_codes else imgs
        out = ops.new((B, self.input_channels, h, w), xin)
        ops.nhwc_to_nchw(xin, out)
        return (out, codes) if return_codes else out


class _PixelChain(_CapturedStep):
    """One position of the chain - every layer's incremental step, the 1x1 output layer, the draw - against static caches,
    captured once (``capture``) and replayed per position, or issued eagerly: the same launches, the same bits."""

    def __init__(self, net: PixelCNN, B: int, temperature: float, codebook_ptr, capture: bool):
        dev = net._flat.device
        super().__init__(net, dev, 1, 1)
        h, w = net.grid
        self.B, self.h, self.w = B, h, w
        Ci, Hd, K = _r4(net.input_channels), _r4(net.hidden_channels), net.output_channels
        self.xin = torch.zeros((B, h, w, Ci), device=dev)
        self.caches = [torch.zeros((B, h, w, Hd), device=dev) for _ in range(len(net.gated_blocks) + 1)]
        self.logits = torch.zeros((B, _r4(K)), device=dev)
        self.codes = torch.zeros((B, h * w), dtype=torch.long, device=dev)
        self.u = torch.zeros(B, device=dev)           # injected uniforms go here
        L, fp = ops.lib(), net._flat
        layers = [(net.input_conv, 0, self.xin, self.caches[0])]
        layers += [(blk.conv, 1, self.caches[i], self.caches[i + 1]) for i, blk in enumerate(net.gated_blocks)]
        g_out = ops.make_geom(B, h, w, Hd, _r4(K), 1, 1, 1, 0)
        need = max([L.lgm_pixelcnn_step_workspace(ctypes.byref(c.geom(B, h, w)), c.taps_live) for c, _, _, _ in layers]
                   + [L.lgm_pixelcnn_step_workspace(ctypes.byref(g_out), 1)])
        self.ws = torch.empty(need // 4, device=dev)
        cb_pitch = 0 if codebook_ptr is None else _r4(net.input_channels)
        oc, cin = net.output_conv, net.input_channels      # the closure keeps no reference to the network (weak cache key)

        def one_step():
            st = ops.stream()
            for conv, gate, src, dst in layers:
                L.lgm_pixelcnn_step(ctypes.byref(conv.geom(B, h, w)), conv.taps_live, gate, src.data_ptr(), ops.pitch(src),
                                    fp.ptr(conv.weight), fp.ptr(conv.bias), self.counter.data_ptr(), dst.data_ptr(),
                                    ops.pitch(dst), 1, self.ws.data_ptr(), need, st)
            L.lgm_pixelcnn_step(ctypes.byref(g_out), 1, 0, self.caches[-1].data_ptr(), Hd, fp.ptr(oc.weight), fp.ptr(oc.bias),
                                self.counter.data_ptr(), self.logits.data_ptr(), _r4(K), 0, self.ws.data_ptr(), need, st)
            u = self.u if self.inject else torch.rand(B, device=dev)
            L.lgm_categorical_draw(self.logits.data_ptr(), _r4(K), B, K, temperature, u.data_ptr(), codebook_ptr, cb_pitch,
                                   cin, h * w, self.counter.data_ptr(), self.codes.data_ptr(),
                                   self.xin.data_ptr(), Ci, 1, st)

        self.one_step = one_step
        self.graphs = None
        if capture:
            self._capture(one_step, (False, True), dev)

    def run(self, uniforms):
        """-> (codes [B, h, w] int64, the input cache [B, h, w, r4(input_channels)]), both copies"""
        self.xin.zero_()
        self.counter.zero_()
        self.inject = uniforms is not None
        if self.inject:
            uniforms = uniforms.to(self.u.device, torch.float32)
        for p in range(self.h * self.w):
            if self.inject:
                self.u.copy_(uniforms[p])
            if self.graphs is not None:
                self.graphs[self.inject].replay()
            else:
                self.one_step()
        return self.codes.view(self.B, self.h, self.w).clone(), self.xin.clone()


class _PixelCNNStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, m: PixelCNN, x4, target):
        save = bool(ctx.needs_input_grad[0])
        mean, logits, tape = m.run(x4, target, save)
        m.last = {"logits": logits}
        ctx.stuff = (m, tape)
        return mean[0]

    @staticmethod
    def backward(ctx, gloss):
        m, tape = ctx.stuff
        if tape is None:
            raise RuntimeError("PixelCNN step ran without saving activations")
        m.backward_hip(tape, gloss.detach().float().reshape(1).contiguous())
        ctx.stuff = None
        return None, None, None, None
