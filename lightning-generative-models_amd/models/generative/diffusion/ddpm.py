"""DDPM / DDIM on the MI355X HIP engine — drop-in for the reference's
``models/generative/diffusion/ddpm.py`` (same class names, constructor arguments, state_dict
keys, ``training_step`` / ``configure_optimizers`` surface).

Nothing here calls ATen compute kernels on the hot path: the UNet forward AND backward are
explicit sequences of liblgm_hip.so launches over NHWC buffers (no autograd graph inside the
network); ``torch.autograd.Function`` is only the seam that lets ``loss.backward()`` of the
Lightning loop trigger the hand-written backward pass.

Reference line anchors are given per class.
"""
from __future__ import annotations

import math
import os
import random
from collections import namedtuple
from typing import List, Optional, Tuple

import torch
from torch import nn

from lgm_hip import ops
from lgm_hip.flat import FlatParams, _r4
from lgm_hip.lightning import LightningModule, multi_rank
from lgm_hip.nn import Conv2d, GradCtx, GroupNorm, Linear, RMSNorm, param_kind
from lgm_hip.optim import EMA, FusedAdam


ModelPrediction = namedtuple("ModelPrediction", ["pred_noise", "pred_x_start"])     # reference :25
# what hip_loss_qsample returns; ``net_t``: the time the network reads where it is not ``t`` (elucidated diffusion: c_noise,
# while ``t`` indexes the loss weights)
QSample = namedtuple("QSample", ["xt", "target", "img", "noise", "t", "offset", "lowres_s", "net_t"], defaults=[None, None])
# The random operands of one training step, in the order a diffusion's ``draw`` takes them from torch's device generator - the
# bits of the loss depend on it, and the graph-replayed step is tested bit for bit against the eager one.  ``t``: the timesteps
# (elucidated diffusion: the normal draw n that sets sigma; None where sigma was given), ``offset``: the [B, C] offset noise,
# ``classes``: the labels as the network gets them (behind the label drop), ``lowres``: (s, eps_aug).  None = the diffusion
# does not have the feature: nothing was drawn for it.
StepDraws = namedtuple("StepDraws", ["t", "noise", "offset", "classes", "dropout_key", "lowres"])


_NO_RES_FOLD = os.environ.get("LGM_NO_RES_FOLD") is not None       # A/B switch: the identity residual's gradient as its own axpby launch


def _chan(t: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    return t[..., lo:hi]


# ----------------------------------------------------------------------------------------
# building blocks  (reference: Block :157-173, ResnetBlock :176-200)
# ----------------------------------------------------------------------------------------
class Block(nn.Module):
    def __init__(self, dim, dim_out, groups=8):
        super().__init__()
        self.proj = Conv2d(dim, dim_out, 3, padding=1)
        self.norm = GroupNorm(groups, dim_out)


class ResnetBlock(nn.Module):
    """conv3x3 -> GN -> FiLM -> SiLU -> [dropout] -> conv3x3 -> GN -> SiLU, + res_conv(x).
    Dropout (extension; Ho et al. 2020, upstream's ``Block(dropout=...)``) acts on ``h1``, the tensor ``block2.proj`` reads:
    ``drop`` = (key address, layer, pass, thr, scale) of ops.gn_fwd, applied inside block1.norm's launches."""

    def __init__(self, dim, dim_out, *, time_emb_dim, groups=8):
        super().__init__()
        self.dim, self.dim_out = dim, dim_out
        self.mlp = nn.Sequential(nn.Identity(), Linear(time_emb_dim, dim_out * 2))
        self.block1 = Block(dim, dim_out, groups)
        self.block2 = Block(dim_out, dim_out, groups)
        self.res_conv = Conv2d(dim, dim_out, 1) if dim != dim_out else nn.Identity()

    def fwd(self, x, ss, out, save: bool, drop=None):
        # a 3x3 convolution that splits its reduction (small maps, small batches) leaves partial planes; the
        # GroupNorm behind it sums them while it computes its statistics: no reducer launch, one round trip less
        G = self.block1.norm.groups
        u1, p1 = self.block1.proj.fwd_planes(x, G)
        h1, sv1 = self.block1.norm.fwd(u1, ss, True, None, planes=p1, drop=drop)
        u2, p2 = self.block2.proj.fwd_planes(h1, G)
        if isinstance(self.res_conv, Conv2d):
            h2, sv2 = self.block2.norm.fwd(u2, None, True, None, planes=p2)
            self.res_conv.fwd(x, out=out, res=h2)
        else:
            _, sv2 = self.block2.norm.fwd(u2, None, True, x, out=out, planes=p2)
        if not save:
            return None
        return (x, ss, u1, sv1, h1, u2, sv2) if drop is None else (x, ss, u1, sv1, h1, u2, sv2, drop)

    def bwd(self, gc: GradCtx, saved, gy, gss, gx, accumulate: bool):
        x, ss, u1, sv1, h1, u2, sv2 = saved[:7]
        drop = saved[7] if len(saved) > 7 else None      # the forward's dropout operands: gh1 goes through the same mask
        # identity residual whose gradient joins a tensor that already holds another branch's (the skip connections of the
        # down path): gx += gy rides in block2's GroupNorm backward, which reads gy anyway (lgm_gn_bwd_add; was an axpby launch)
        fold_res = accumulate and not isinstance(self.res_conv, Conv2d) and not _NO_RES_FOLD
        gu2 = self.block2.norm.bwd(gc, u2, gy, None, True, sv2, None, add_gy_to=gx if fold_res else None)
        gh1, pg = self.block2.proj.bwd(gc, h1, gu2, planes_for_groups=self.block1.norm.groups)
        del gu2
        gu1 = self.block1.norm.bwd(gc, u1, gh1, ss, True, sv1, gss, gy_planes=pg, drop=drop)
        del gh1
        if isinstance(self.res_conv, Conv2d):
            self.block1.proj.bwd(gc, x, gu1, gx, accumulate)
            self.res_conv.bwd(gc, x, gy, gx, True)
        elif accumulate:
            if not fold_res:
                ops.axpby(gx, 1.0, gy, 1.0, gx)
            self.block1.proj.bwd(gc, x, gu1, gx, True)
        else:
            self.block1.proj.bwd(gc, x, gu1, gx, False, res=gy)
        return gx


class LinearAttention(nn.Module):
    """reference :203-239"""

    def __init__(self, dim, heads=4, dim_head=32, num_mem_kv=4):
        super().__init__()
        self.heads, self.dim_head, self.M = heads, dim_head, num_mem_kv
        hidden = heads * dim_head
        self.norm = RMSNorm(dim)
        self.mem_kv = nn.Parameter(torch.randn(2, heads, dim_head, num_mem_kv))
        self.to_qkv = Conv2d(dim, hidden * 3, 1, bias=False)
        self.to_out = nn.Sequential(Conv2d(hidden, dim, 1), RMSNorm(dim))

    def fwd(self, x, out, save: bool):
        """out = attn(x) + x"""
        B, H, W, C = x.shape
        fp = self.mem_kv._lgm_flat
        r = ops.rms_qkv_fused(x, fp.ptr(self.norm.g), fp.ptr(self.to_qkv.weight), 3 * self.heads * self.dim_head)
        if r is not None:
            xn, qkv = r                                  # RMSNorm + to_qkv in one launch
        else:
            xn = self.norm.fwd(x)
            qkv = self.to_qkv.fwd(xn)
        ao = ops.new((B, H, W, self.heads * self.dim_head), x)
        conv, norm = self.to_out[0], self.to_out[1]
        if ops.linattn_fwd_fused_ok(self.heads, self.dim_head, C, qkv, x, fp.ptr(conv.weight), fp.ptr(conv.bias),
                                    fp.ptr(norm.g)) and out.data_ptr() % 16 == 0 and ops.pitch(out) % 4 == 0:
            # softmax_d(q) ctx -> to_out[0] -> RMSNorm -> + x in one launch behind the context launch
            o2 = ops.new((B, H, W, C), x)
            ctx, kstat = ops.linattn_fwd_fused(qkv, fp.ptr(self.mem_kv), self.heads, self.dim_head, self.M,
                                               fp.ptr(conv.weight), fp.ptr(conv.bias), fp.ptr(norm.g), x, ao, o2, out)
        else:
            ctx, kstat = ops.linattn_fwd(qkv, fp.ptr(self.mem_kv), self.heads, self.dim_head, self.M, ao)
            o2 = conv.fwd(ao)
            norm.fwd(o2, res=x, out=out)
        return (x, xn, qkv, ao, ctx, kstat, o2) if save else None

    def bwd(self, gc: GradCtx, saved, gy, gx, accumulate: bool):
        x, xn, qkv, ao, ctx, kstat, o2 = saved
        fp = gc.flat
        go2 = self.to_out[1].bwd(gc, o2, gy)
        gao = self.to_out[0].bwd(gc, ao, go2)
        del go2
        w = self.to_qkv.weight
        gqkv = None
        if ops.linattn_bwd_fused_ok(self.heads, self.dim_head, xn.shape[-1], qkv, gao, xn, fp.tptr(w), fp.gptr(w),
                                    fp.gptr(self.mem_kv)):
            # large maps: gq / gk / gv never reach memory - the kernel that computes them also multiplies them
            # with to_qkv's weight (input gradient) and with xn (weight gradient)
            dw, dm = gc.defer_for(w), gc.defer_for(self.mem_kv)
            bw, bm = gc.beta(w), gc.beta(self.mem_kv)
            gxn = ops.new(xn.shape, xn)
            ops.linattn_bwd_fused(qkv, fp.ptr(self.mem_kv), gao, ctx, kstat, xn, fp.tptr(w), self.heads, self.dim_head,
                                  self.M, gxn, fp.gptr(w), bw, dw, fp.gptr(self.mem_kv), bm, dm)
        else:
            gqkv = ops.new(qkv.shape, qkv)
            dm = gc.defer_for(self.mem_kv)
            ops.linattn_bwd(qkv, fp.ptr(self.mem_kv), gao, ctx, kstat, self.heads, self.dim_head, self.M, gqkv,
                            fp.gptr(self.mem_kv), gc.beta(self.mem_kv), defer=dm)
            gxn = self.to_qkv.bwd(gc, xn, gqkv)
        del gqkv, gao
        # gx (+)= d norm / dx + gy: the residual branch's gradient rides in the RMSNorm backward pass
        self.norm.bwd(gc, x, gxn, gx, accumulate, res=gy)
        return gx


class Attention(nn.Module):
    """reference :242-271 (+ modules/attend.py:97-126)"""

    def __init__(self, dim, heads=4, dim_head=32, num_mem_kv=4, flash=False):
        super().__init__()
        self.heads, self.dim_head, self.M = heads, dim_head, num_mem_kv
        hidden = heads * dim_head
        self.norm = RMSNorm(dim)
        self.mem_kv = nn.Parameter(torch.randn(2, heads, num_mem_kv, dim_head))
        self.to_qkv = Conv2d(dim, hidden * 3, 1, bias=False)
        self.to_out = Conv2d(hidden, dim, 1)

    def fwd(self, x, out, save: bool):
        B, H, W, C = x.shape
        fp = self.mem_kv._lgm_flat
        r = ops.rms_qkv_fused(x, fp.ptr(self.norm.g), fp.ptr(self.to_qkv.weight), 3 * self.heads * self.dim_head)
        if r is not None:
            xn, qkv = r                                  # RMSNorm + to_qkv in one launch
        else:
            xn = self.norm.fwd(x)
            qkv = self.to_qkv.fwd(xn)
        ao = ops.new((B, H, W, self.heads * self.dim_head), x)
        lse = ops.attn_fwd(qkv, fp.ptr(self.mem_kv), self.heads, self.dim_head, self.M, ao)
        self.to_out.fwd(ao, out=out, res=x)
        return (x, xn, qkv, ao, lse) if save else None

    def bwd(self, gc: GradCtx, saved, gy, gx, accumulate: bool):
        x, xn, qkv, ao, lse = saved
        fp = gc.flat
        gao = self.to_out.bwd(gc, ao, gy)
        gqkv = ops.new(qkv.shape, qkv)
        dm = gc.defer_for(self.mem_kv)
        ops.attn_bwd(qkv, fp.ptr(self.mem_kv), ao, gao, lse, self.heads, self.dim_head, self.M, gqkv,
                     fp.gptr(self.mem_kv), gc.beta(self.mem_kv), defer=dm)
        gxn = self.to_qkv.bwd(gc, xn, gqkv)
        del gqkv, gao
        # gx (+)= d norm / dx + gy: the residual branch's gradient rides in the RMSNorm backward pass
        self.norm.bwd(gc, x, gxn, gx, accumulate, res=gy)
        return gx


class _DownConv(Conv2d):
    """The convolution of ``Downsample`` (:100-104: ``Rearrange('b c (h p1) (w p2) -> b (c p1 p2) h w')`` + ``Conv2d(4 C, N, 1)``)
    as what the two are together: a 2 x 2 / stride-2 convolution of the un-shuffled tensor (the index shuffle lives
    in the convolution's gather, nothing is materialised).  The parameter is held as ``[N, C, 2, 2]``; its row-major
    flattening IS the reference's ``[N, 4 C, 1, 1]`` weight (input channel ``c p1 p2`` = ``4 c + 2 p1 + p2``), same fan-in, same
    initialisation stream.  ``state_dict()`` / ``load_state_dict()`` and the optimizer's checkpoint state exchange the
    reference's shape (``ParamSlot.ref_shape``)."""

    def __init__(self, dim, dim_out):
        super().__init__(dim, dim_out, 2, stride=2, padding=0)

    @property
    def ref_shape(self):
        return (self.cout, 4 * self.cin, 1, 1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        k = prefix + "weight"
        destination[k] = destination[k].reshape(self.ref_shape)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        k = prefix + "weight"
        w = state_dict.get(k)
        if w is not None and tuple(w.shape) == self.ref_shape:
            state_dict = {kk: v for kk, v in state_dict.items() if kk.startswith(prefix)}
            state_dict[k] = w.reshape(self.weight.shape)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class _Down(nn.Module):
    """Downsample (:100-104): pixel-unshuffle + 1x1 conv = one 2x2 / stride-2 convolution (``_DownConv``); keys
    ``<idx>.1.weight`` / ``<idx>.1.bias``."""

    def __init__(self, dim, dim_out):
        super().__init__()
        self.add_module("0", nn.Identity())
        self.add_module("1", _DownConv(dim, dim_out))

    def fwd(self, x, out, save):
        self._modules["1"].fwd(x, out=out)
        return (x,) if save else None

    def bwd(self, gc, saved, gy, gx, accumulate):
        (x,) = saved
        self._modules["1"].bwd(gc, x, gy, gx, accumulate)
        return gx


class _Up(nn.Module):
    """Upsample (:93-97): nearest x2 + conv3x3; keys ``<idx>.1.weight``."""

    def __init__(self, dim, dim_out):
        super().__init__()
        self.add_module("0", nn.Identity())
        self.add_module("1", Conv2d(dim, dim_out, 3, padding=1))

    def fwd(self, x, out, save):
        B, H, W, C = x.shape
        hi = ops.new((B, 2 * H, 2 * W, C), x)
        ops.upsample2x_fwd(x, hi)
        self._modules["1"].fwd(hi, out=out)
        return (hi,) if save else None

    def bwd(self, gc, saved, gy, gx, accumulate):
        (hi,) = saved
        ghi = self._modules["1"].bwd(gc, hi, gy)
        ops.upsample2x_bwd(ghi, gx, accumulate)
        return gx


class FourierPosEmb(nn.Module):
    """RandomOrLearnedSinusoidalPosEmb (:135-151): the parameter alone, key ``time_mlp.0.weights`` [dim / 2]; the row is
    written by ``lgm_fourier_emb_fwd`` (``Unet._emb_mlp_fwd``)."""

    def __init__(self, dim, is_random=False):
        super().__init__()
        self.is_random = bool(is_random)
        self.weights = nn.Parameter(torch.randn(dim // 2), requires_grad=not is_random)


class _PlainConv(Conv2d):
    """Last-stage 3x3 conv used in place of Down/Up (:377, :413)."""

    def fwd_s(self, x, out, save):
        self.fwd(x, out=out)
        return (x,) if save else None

    def bwd_s(self, gc, saved, gy, gx, accumulate):
        (x,) = saved
        self.bwd(gc, x, gy, gx, accumulate)
        return gx


# ----------------------------------------------------------------------------------------
# UNet  (reference :275-471)
# ----------------------------------------------------------------------------------------
class Unet(nn.Module):
    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=3,
                 self_condition=False, resnet_block_groups=8, learned_variance=False,
                 learned_sinusoidal_cond=False, random_fourier_features=False,
                 learned_sinusoidal_dim=16, sinusoidal_pos_emb_theta=10000, attn_dim_head=32,
                 attn_heads=4, full_attn=None, flash_attn=False, num_classes=None, dropout=0.0, lowres_cond=False):
        """``dropout`` (extension, like upstream's ``Unet(dropout=...)``): the probability with which every ResnetBlock drops
        the elements of ``h1`` in the network passes of the training loss (``forward_nhwc(dropout_key=...)``; nothing else
        ever drops).  No parameters, no buffers: state-dict keys and parameter order are those of a model without it.
        ``lowres_cond`` (extension; a super-resolution stage of a cascade - SR3, Cascaded Diffusion Models, Imagen): the network
        reads ``cat((lowres_cond_img, x), dim=1)``, the conditioning image already at x's size, and adds ``lowres_time_mlp(s)``
        - an embedding of the conditioning image's noise-augmentation level s with the structure of ``time_mlp``, Imagen's
        ``to_lowres_time_hiddens`` - to the time embedding.  ``init_conv.weight`` is [dim, 2 C, 7, 7] and every other key is
        that of the reference's self-conditioned Unet, plus ``lowres_time_mlp.*``.
        ``learned_sinusoidal_cond`` / ``random_fourier_features`` / ``learned_sinusoidal_dim`` (the reference's, :315-326): the
        network embeds a REAL-valued time - float32 [B] in ``forward`` / ``forward_nhwc`` / ``forward_guided`` - through
        ``time_mlp.0.weights`` [learned_sinusoidal_dim / 2], trained when learned and a saved constant when random; what
        ``ElucidatedDiffusion`` (edm.py) is built around.  NotImplementedError together with ``self_condition``,
        ``learned_variance`` or ``lowres_cond``."""
        super().__init__()
        if lowres_cond and self_condition:
            raise NotImplementedError("lowres_cond together with self_condition is not built: both would take the first C "
                                      "input channels of init_conv")
        self.drop_thr, self.drop_scale = ops.dropout_operands(dropout)      # ValueError outside [0, 1)
        self.dropout = float(dropout)
        if num_classes is not None and int(num_classes) < 1:
            raise ValueError(f"num_classes must be a positive number of classes, got {num_classes!r}")
        fourier = bool(learned_sinusoidal_cond or random_fourier_features)
        if fourier and (self_condition or learned_variance or lowres_cond):
            # tests/test_selfcond_host.py and tests/test_learned_sigma_host.py pin the first two refusals
            raise NotImplementedError("the random / learned fourier time embedding together with self_condition, "
                                      "learned_variance or lowres_cond is not built")
        if fourier and (int(learned_sinusoidal_dim) < 2 or int(learned_sinusoidal_dim) % 2):
            raise ValueError(f"learned_sinusoidal_dim must be a positive even number, got {learned_sinusoidal_dim!r}")
        if learned_variance and self_condition:
            # tests/test_selfcond_host.py pins this refusal; the hybrid loss's estimate pass is not built for the combination
            raise NotImplementedError("learned_variance together with self_condition is not built")
        if init_dim not in (None, dim):
            raise NotImplementedError("init_dim != dim")
        self.dim, self.channels = dim, channels
        # learned variance (:417-418): out_dim = 2 C; lanes [0, C) of the NHWC output are the objective's prediction, lanes
        # [C, 2 C) the interpolation coefficient v of the model's log-variance (Nichol & Dhariwal 2021, eq. 15)
        self.learned_variance = bool(learned_variance)
        self.self_condition = bool(self_condition)
        self.lowres_cond = bool(lowres_cond)
        # the reference's RandomOrLearnedSinusoidalPosEmb (:135-151, 315-326): the network reads a REAL-valued time (float32 [B])
        # through the row (x, sin(2 pi x w), cos(2 pi x w)) of learned_sinusoidal_dim + 1 lanes; ``weights`` is trained when
        # learned and a constant - never written by the optimizer, copied by the EMA, saved - when random
        self.random_or_learned_sinusoidal_cond = fourier
        self.fourier_half = int(learned_sinusoidal_dim) // 2 if fourier else 0
        self.theta = float(sinusoidal_pos_emb_theta)
        # self-conditioned (:300-301, 435): the network reads cat((x_self_cond, x), dim=1) - ONE NHWC buffer of r4(2 C) lanes
        # whose slices [sc_off, sc_off + C) and [x_off, x_off + C) their producers fill; nothing is concatenated
        # low-resolution conditioned: the same layout with the conditioning image where x_self_cond would stand - a CONSTANT
        # slice [cond_off, cond_off + C), written once per training step / sampling chain by lgm_lowres_cond; the kernels that
        # rewrite x own the lanes from x_off on (``x_extent``) and never touch it
        self.in_channels = channels * (2 if self.self_condition or self.lowres_cond else 1)
        self.in_pitch = _r4(self.in_channels)
        self.x_off, self.sc_off = (channels, 0) if self.self_condition else (channels, -1) if self.lowres_cond else (0, -1)
        self.cond_off = 0 if self.lowres_cond else -1
        self.init_conv = Conv2d(self.in_channels, dim, 7, padding=3)
        dims = [dim, *[dim * m for m in dim_mults]]
        in_out = list(zip(dims[:-1], dims[1:]))
        self.in_out = in_out
        time_dim = dim * 4
        self.time_dim = time_dim
        if fourier:
            self.time_mlp = nn.Sequential(FourierPosEmb(int(learned_sinusoidal_dim), bool(random_fourier_features)),
                                          Linear(int(learned_sinusoidal_dim) + 1, time_dim), nn.Identity(),
                                          Linear(time_dim, time_dim))
        else:
            self.time_mlp = nn.Sequential(nn.Identity(), Linear(dim, time_dim), nn.Identity(), Linear(time_dim, time_dim))
        # class-conditional (extension): temb = time_mlp(t) + label_emb.weight[classes], row num_classes = the null label
        # classifier-free guidance trains and samples with; N(0, 1) like nn.Embedding, dense under Adam and the EMA
        self.num_classes = None if num_classes is None else int(num_classes)
        if self.num_classes is not None:
            self.label_emb = nn.Embedding(self.num_classes + 1, time_dim)
        self._null_labels = {}
        if self.lowres_cond:
            self.lowres_time_mlp = nn.Sequential(nn.Identity(), Linear(dim, time_dim), nn.Identity(), Linear(time_dim, time_dim))
        n = len(in_out)
        if not full_attn:
            full_attn = (*((False,) * (n - 1)), True)
        heads = attn_heads if isinstance(attn_heads, tuple) else (attn_heads,) * n
        dheads = attn_dim_head if isinstance(attn_dim_head, tuple) else (attn_dim_head,) * n
        rb = lambda a, b: ResnetBlock(a, b, time_emb_dim=time_dim, groups=resnet_block_groups)  # noqa: E731
        self.downs = nn.ModuleList([])
        self.ups = nn.ModuleList([])
        for i, ((ci, co), fa, h, dh) in enumerate(zip(in_out, full_attn, heads, dheads)):
            last = i >= n - 1
            att = Attention(ci, heads=h, dim_head=dh) if fa else LinearAttention(ci, heads=h, dim_head=dh)
            self.downs.append(nn.ModuleList([rb(ci, ci), rb(ci, ci), att,
                                             _Down(ci, co) if not last else _PlainConv(ci, co, 3, padding=1)]))
        mid = dims[-1]
        self.mid_block1 = rb(mid, mid)
        self.mid_attn = Attention(mid, heads=heads[-1], dim_head=dheads[-1])
        self.mid_block2 = rb(mid, mid)
        for i, ((ci, co), fa, h, dh) in enumerate(zip(*map(reversed, (in_out, full_attn, heads, dheads)))):
            last = i == n - 1
            att = Attention(co, heads=h, dim_head=dh) if fa else LinearAttention(co, heads=h, dim_head=dh)
            self.ups.append(nn.ModuleList([rb(co + ci, co), rb(co + ci, co), att,
                                           _Up(co, ci) if not last else _PlainConv(co, ci, 3, padding=1)]))
        self.out_dim = out_dim if out_dim is not None else channels * (2 if self.learned_variance else 1)
        self.final_res_block = rb(dim * 2, dim)
        self.final_conv = Conv2d(dim, self.out_dim, 1)
        self._flat: Optional[FlatParams] = None

    # ---- flat storage ---------------------------------------------------------------------
    def resblocks(self) -> List[ResnetBlock]:
        out = []
        for b1, b2, _, _ in self.downs:
            out += [b1, b2]
        out += [self.mid_block1, self.mid_block2]
        for b1, b2, _, _ in self.ups:
            out += [b1, b2]
        out.append(self.final_res_block)
        return out

    def __deepcopy__(self, memo):
        # EMA shadow copies must get their own flat storage: copy with plain (unbound) parameters
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_flat":
                new.__dict__[k] = None
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        for p in new.parameters():
            p.data = p.data.contiguous().clone()
        return new

    def prepare_hip(self, device) -> FlatParams:
        """Bind all parameters to flat device storage (idempotent)."""
        device = torch.device(device)
        if self._flat is not None and self._flat.device == device and self._flat.still_bound():
            return self._flat
        named = dict(self.named_parameters())
        rbs = self.resblocks()
        first: List[Tuple[str, nn.Parameter, str]] = []
        names = {id(p): n for n, p in named.items()}
        for rb in rbs:   # the 2C x time_dim FiLM projections become ONE [sum(2C), time_dim] GEMM operand
            first.append((names[id(rb.mlp[1].weight)], rb.mlp[1].weight, "weight"))
        for rb in rbs:
            first.append((names[id(rb.mlp[1].bias)], rb.mlp[1].bias, "vector"))
        for lin in (self.time_mlp[1], self.time_mlp[3]):      # their gradients are produced last, too
            first.append((names[id(lin.weight)], lin.weight, "weight"))
            first.append((names[id(lin.bias)], lin.bias, "vector"))
        if self.random_or_learned_sinusoidal_cond:            # the fourier frequencies: their gradient ends the time phase
            first.append((names[id(self.time_mlp[0].weights)], self.time_mlp[0].weights, "vector"))
        if self.num_classes is not None:                      # dense rows [K + 1, time_dim], final with the time MLP's
            first.append((names[id(self.label_emb.weight)], self.label_emb.weight, "vector"))
        if self.lowres_cond:                                  # the augmentation-level MLP: backward with the time MLP's
            for lin in (self.lowres_time_mlp[1], self.lowres_time_mlp[3]):
                first.append((names[id(lin.weight)], lin.weight, "weight"))
                first.append((names[id(lin.bias)], lin.bias, "vector"))
        taken = {id(p) for _, p, _ in first}
        rest = [(n, p, param_kind(n, p)) for n, p in named.items() if id(p) not in taken]
        self._flat = FlatParams(first + rest, device)
        for m in self.modules():
            if isinstance(m, _DownConv):       # checkpoints exchange this weight as the reference's [N, 4 C, 1, 1]
                self._flat.slot(m.weight).ref_shape = m.ref_shape
        if ops.B3:                     # opt-in split-precision 3x3 convolutions (LGM_CONV_MODE=bf16x3)
            self._flat.enable_b3()
        elif ops.WINO:                 # Winograd F(2x2,3x3) in exact fp32 arithmetic for the 3x3 layers
            self._flat.enable_wino()
        # gradient-exchange buckets in backward completion order: [ups, mid, final] -> [init_conv, downs]
        # -> [FiLM + time MLP]  (registration order of `rest`: init_conv, downs, ups, mid_*, final_*)
        slots = {s.name: s for s in self._flat.slots}
        self._head_end = slots[rest[0][0]].offset
        rest_names = [n for n, _, _ in rest]
        self._ups_start = min(slots[n].offset for n in rest_names if n.startswith("ups."))
        self._mid_start = min(slots[n].offset for n in rest_names if n.startswith("mid_"))
        self._final_start = min(slots[n].offset for n in rest_names if n.startswith("final_"))
        assert self._ups_start < self._mid_start < self._final_start
        assert all(self._ups_start <= slots[n].offset < self._mid_start for n in rest_names if n.startswith("ups."))
        assert all(self._mid_start <= slots[n].offset < self._final_start for n in rest_names if n.startswith("mid_"))
        assert all(slots[n].offset >= self._final_start for n in rest_names if n.startswith("final_"))
        assert all(slots[n].offset >= self._ups_start for n in rest_names
                   if n.startswith(("ups.", "mid_", "final_")))
        assert all(self._head_end <= slots[n].offset < self._ups_start for n in rest_names
                   if n.startswith(("downs.", "init_conv")))
        self.grad_sync = None
        self._ss_offsets = []
        off = 0
        for rb in rbs:
            self._ss_offsets.append(off)
            off += 2 * rb.dim_out
        self._ss_total = off
        self._mlp_geoms = {}
        return self._flat

    # ---- time embedding -------------------------------------------------------------------
    def labels(self, classes, B, device):
        """The int64 [B] device tensor of labels the kernels read, or None for a network without classes.  ``None`` on a
        class-conditional network = the null label for every sample.  Labels the host can see (a CPU tensor, a list) are
        checked against [0, num_classes]; labels already on the device are clamped by the kernels."""
        K = self.num_classes
        if K is None:
            if classes is not None:
                raise ValueError("classes were passed to a Unet built without num_classes")
            return None
        device = torch.device(device)
        if classes is None:
            key = (B, device)
            y = self._null_labels.get(key)
            if y is None:
                y = self._null_labels[key] = torch.full((B,), K, dtype=torch.long, device=device)
            return y
        y = torch.as_tensor(classes)
        if y.dtype.is_floating_point or y.dtype == torch.bool or tuple(y.shape) != (B,):
            raise ValueError(f"classes must be {B} integer labels (one per sample), got {y.dtype} {tuple(y.shape)}")
        if y.device.type == "cpu" and B > 0 and (int(y.min()) < 0 or int(y.max()) > K):
            raise ValueError(f"classes must lie in [0, {K}] ({K} = the null label), got [{int(y.min())}, {int(y.max())}]")
        return y.to(device=device, dtype=torch.long).contiguous()

    def aug_levels(self, lowres_aug_t, B, device):
        """The int64 [B] device tensor of augmentation levels ``lowres_time_mlp`` embeds, or None for a network without
        low-resolution conditioning.  ``None`` on a conditioned network = level 0 (no augmentation) for every sample; an int
        = that level for every sample."""
        if not self.lowres_cond:
            if lowres_aug_t is not None:
                raise ValueError("lowres_aug_t was passed to a Unet built without lowres_cond")
            return None
        if lowres_aug_t is None or isinstance(lowres_aug_t, int):
            return torch.full((B,), int(lowres_aug_t or 0), dtype=torch.long, device=device)
        s = torch.as_tensor(lowres_aug_t)
        if s.dtype.is_floating_point or s.dtype == torch.bool or tuple(s.shape) != (B,):
            raise ValueError(f"lowres_aug_t must be {B} integer levels (one per sample), got {s.dtype} {tuple(s.shape)}")
        return s.to(device=device, dtype=torch.long).contiguous()

    def _emb_mlp_fwd(self, mlp, t, out=None):
        """``time_mlp`` / ``lowres_time_mlp`` over the integer input ``t`` on the unfused ops: posemb, linear, GELU, linear
        (four launches) -> (pe, a1, h, emb), in ``out`` where the caller owns the four buffers"""
        B, fp = t.shape[0], self._flat
        l1, l2 = mlp[1], mlp[3]
        pe, a1, h, emb = out or (ops.new((B, d), t) for d in (self._pe_width(mlp), self.time_dim, self.time_dim, self.time_dim))
        if self._is_fourier(mlp):
            # the real-valued time's row at the pitch ``l1.geom`` reads (r4(learned_sinusoidal_dim + 1) lanes, padding zero)
            ops.fourier_emb_fwd(t, fp.ptr(mlp[0].weights), self.fourier_half, pe)
        else:
            ops.posemb(t, self.dim, self.theta, pe)
        ops.conv_xy(l1.geom(B), pe, fp.ptr(l1.weight), fp.ptr(l1.bias), None, a1)
        ops.act_fwd(a1, None, None, h, ops.ACT_GELU)
        ops.conv_xy(l2.geom(B), h, fp.ptr(l2.weight), fp.ptr(l2.bias), None, emb)
        return pe, a1, h, emb

    def _is_fourier(self, mlp) -> bool:
        """``mlp`` is the time MLP of a network with the random / learned fourier embedding (``lowres_time_mlp`` never is)"""
        return self.random_or_learned_sinusoidal_cond and mlp is self.time_mlp

    def _pe_width(self, mlp) -> int:
        return _r4(2 * self.fourier_half + 1) if self._is_fourier(mlp) else self.dim

    def _time_mlp_fused(self) -> bool:
        """The time MLP runs on the fused sinusoidal kernels (``lgm_time_mlp_fwd`` / ``_bwd``, opt-in).  ONE decision for the forward
        and the backward: a network with the fourier embedding never does, whatever the switch says - those kernels embed an
        integer time and read a [B, dim] row, its row is [B, r4(learned_sinusoidal_dim + 1)]."""
        if self.random_or_learned_sinusoidal_cond:
            return False
        return ops.time_mlp_ok(self.dim, self.time_dim, self.time_mlp[1], self.time_mlp[3])

    def check_time(self, time):
        """TypeError by name unless ``time`` has the type this network embeds: float32 [B] with the fourier embedding (a
        real-valued time), an integer tensor with the sinusoidal one"""
        if self.random_or_learned_sinusoidal_cond:
            if not torch.is_tensor(time) or not time.dtype.is_floating_point:
                raise TypeError("a Unet with the random / learned fourier embedding takes a floating-point time [B], got "
                                f"{time.dtype if torch.is_tensor(time) else type(time).__name__}")
            return time.detach().to(torch.float32).contiguous()
        if not torch.is_tensor(time) or time.dtype.is_floating_point:
            raise TypeError("a Unet with the sinusoidal embedding takes an integer time [B], got "
                            f"{time.dtype if torch.is_tensor(time) else type(time).__name__}")
        return time

    def _time_fwd(self, t, save, classes=None, lowres_s=None):
        B = t.shape[0]
        fp = self._flat
        l1, l2 = self.time_mlp[1], self.time_mlp[3]
        pe = ops.new((B, self._pe_width(self.time_mlp)), t)
        a1 = ops.new((B, self.time_dim), t)
        h = ops.new((B, self.time_dim), t)
        temb = ops.new((B, self.time_dim), t)
        st = ops.new((B, self.time_dim), t)
        if self._time_mlp_fused():
            # posemb -> Linear -> GELU -> Linear -> SiLU in ONE launch (was six: csrc/elementwise.hip time_mlp_fwd_kernel)
            ops.time_mlp_fwd(t, self.dim, self.theta, fp.ptr(l1.weight), fp.ptr(l1.bias), fp.ptr(l2.weight),
                             fp.ptr(l2.bias), self.time_dim, pe, a1, h, temb, st)
        else:
            self._emb_mlp_fwd(self.time_mlp, t, (pe, a1, h, temb))
            if self.num_classes is None and not self.lowres_cond:
                ops.act_fwd(temb, None, None, st, ops.ACT_SILU)
        lowres = None
        if self.lowres_cond:
            # temb += lowres_time_mlp(s), st = SiLU(temb): the MLP on the unfused ops and one row-local launch that joins it
            # to the time embedding
            assert lowres_s is not None, "a low-resolution conditioned network needs its augmentation levels"
            pe_s, a1_s, h_s, emb_s = self._emb_mlp_fwd(self.lowres_time_mlp, lowres_s)
            ops.lowres_emb_fwd(temb, None if self.num_classes is not None else st, emb_s)
            lowres = (pe_s, a1_s, h_s)
        if self.num_classes is not None:
            # temb += label_emb[classes], st = SiLU(temb): one row-local launch behind the time MLP
            classes = self.labels(None, B, t.device) if classes is None else classes
            ops.label_emb_fwd(temb, st, fp.ptr(self.label_emb.weight), classes, self.num_classes)
        g = self._mlp_geoms.get(B)
        if g is None:
            g = ops.make_geom(B, 1, 1, self.time_dim, self._ss_total, 1, 1, 1, 0)
            self._mlp_geoms[B] = g
        rb0 = self.resblocks()[0]
        ss_all = ops.new((B, self._ss_total), t)
        ops.conv_xy(g, st, fp.ptr(rb0.mlp[1].weight), fp.ptr(rb0.mlp[1].bias), None, ss_all)
        return ss_all, (TimeTape(pe, a1, h, temb, st, classes, lowres) if save else None)

    def _time_bwd(self, gc: GradCtx, saved: "TimeTape", gss_all):
        st = saved.st
        B = st.shape[0]
        fp = gc.flat
        l1, l2 = self.time_mlp[1], self.time_mlp[3]
        rbs = self.resblocks()
        g = self._mlp_geoms[B]
        ops.conv_wgrad(g, gss_all, st, fp.gptr(rbs[0].mlp[1].weight), gc.beta0, fp.gptr(rbs[0].mlp[1].bias))
        for rb in rbs:
            gc.written.add(id(rb.mlp[1].weight))
            gc.written.add(id(rb.mlp[1].bias))
        gst = ops.new(st.shape, st)
        ops.conv_yx(g, gss_all, fp.ptr(rbs[0].mlp[1].weight), None, None, gst)
        gtemb = ops.new(st.shape, st)
        fused = self._time_mlp_fused()           # the forward's decision: the tape holds what that path saved
        if fused:
            # SiLU' -> (weight / bias gradient, input gradient) of the second linear -> GELU' -> weight / bias gradient of the
            # first: two launches (row-local chain, batch reductions in row order) instead of six
            bw = gc.beta(l2.weight)
            assert bw == gc.beta(l2.bias) == gc.beta(l1.weight) == gc.beta(l1.bias)
            ga1 = ops.new(saved.a1.shape, saved.a1)
            ops.time_mlp_bwd(gst, saved.pe, saved.a1, saved.h, saved.temb, fp.ptr(l2.weight), self.dim, self.time_dim, gtemb,
                             ga1, fp.gptr(l1.weight), fp.gptr(l1.bias), fp.gptr(l2.weight), fp.gptr(l2.bias), bw)
        else:
            ops.act_bwd(saved.temb, None, gst, gtemb, False, ops.ACT_SILU)
        self._label_emb_bwd(gc, gtemb, saved.classes)
        self._lowres_mlp_bwd(gc, gtemb, saved.lowres)
        if not fused:
            ga1 = self._emb_mlp_bwd(gc, self.time_mlp, gtemb, saved.pe, saved.a1, saved.h)
            pos = self.time_mlp[0]
            if self.random_or_learned_sinusoidal_cond and not pos.is_random:
                # learned frequencies: the first linear's input gradient, then g_w summed over the batch in row order by one
                # workgroup (the forward's own row holds x, sin and cos).  Random features get no launch: their gradient
                # slot stays zero, and Adam leaves a parameter with m = v = g = 0 as it is.
                l1 = self.time_mlp[1]
                gpe = ops.new(saved.pe.shape, saved.pe)
                ops.conv_yx(l1.geom(B), ga1, fp.ptr(l1.weight), None, None, gpe, wt_ptr=fp.tptr(l1.weight))
                ops.fourier_emb_bwd(saved.pe, gpe, self.fourier_half, fp.gptr(pos.weights), gc.beta(pos.weights))

    def _emb_mlp_bwd(self, gc: GradCtx, mlp, gemb, pe, a1, h):
        """The backward of ``_emb_mlp_fwd`` from the gradient of its output: weight + input gradient of the second linear in
        one launch (lgm_conv_bwd_pair), GELU', weight gradient of the first."""
        B, fp = pe.shape[0], gc.flat
        l1, l2 = mlp[1], mlp[3]
        gh = ops.new(h.shape, h)
        ops.conv_bwd_generic(l2.geom(B), gemb, h, fp.ptr(l2.weight), fp.tptr(l2.weight), fp.gptr(l2.weight),
                             gc.beta(l2.weight), fp.gptr(l2.bias), None, None, gh)
        gc.beta(l2.bias)
        ga1 = ops.new(a1.shape, a1)
        ops.act_bwd(a1, None, gh, ga1, False, ops.ACT_GELU)
        ops.conv_wgrad(l1.geom(B), ga1, pe, fp.gptr(l1.weight), gc.beta(l1.weight), fp.gptr(l1.bias))
        gc.beta(l1.bias)
        return ga1

    def _lowres_mlp_bwd(self, gc: GradCtx, gtemb, lowres):
        """temb is a sum: g lowres_time_mlp(s) = g temb"""
        if lowres is not None:
            self._emb_mlp_bwd(gc, self.lowres_time_mlp, gtemb, *lowres)

    def _label_emb_bwd(self, gc: GradCtx, gtemb, classes):
        """g label_emb.weight[k] = sum of g temb[b] over the samples of class k, in ascending b; other rows exactly zero"""
        if self.num_classes is not None:
            w = self.label_emb.weight
            ops.label_emb_wgrad(gtemb, classes, gc.flat.gptr(w), gc.beta(w), self.num_classes)

    # ---- network ----------------------------------------------------------------------------
    def forward_guided(self, x, t, classes=None, cond_scale: float = 1.0, refresh_weights: bool = True, scale_dev=None,
                       lowres_s=None):
        """The network output a sampler reads (no saved activations).  ``cond_scale == 1``: one forward with ``classes``.
        Otherwise classifier-free guidance: a second forward over the SAME input buffer with the null label, then
        out = out_null + cond_scale * (out - out_null) in place (lgm_cfg_mix); the derived weights are refreshed once.
        ``scale_dev``: a device float holding the scale (captured steps), which makes the step a guided one.
        ``lowres_s``: the augmentation levels of a low-resolution conditioned network (``aug_levels``), both forwards' alike."""
        out, _ = self.forward_nhwc(x, t, False, refresh_weights, classes, lowres_s=lowres_s)
        if scale_dev is not None or float(cond_scale) != 1.0:
            if self.num_classes is None:
                raise ValueError("cond_scale != 1 needs a Unet built with num_classes")
            null, _ = self.forward_nhwc(x, t, False, False, None, lowres_s=lowres_s)
            # a learned-variance network mixes its prediction lanes alone: the variance of a guided step is the conditional
            # forward's (lanes [C, 2 C) of ``out`` stay as that forward wrote them)
            ops.cfg_mix(out, null, cond_scale, self.channels if self.learned_variance else self.out_dim, scale_dev)
        return out

    def drop_operands(self, dropout_key, drop_pass: int):
        """Per resblock (``resblocks()`` order = the mask's ``layer``) the dropout operands of ops.gn_fwd, or None each when
        this pass does not drop: no key, ``dropout == 0`` or evaluation mode."""
        n = len(self.resblocks())
        if dropout_key is None or self.dropout <= 0.0 or not self.training:
            return [None] * n
        assert dropout_key.dtype == torch.int64 and dropout_key.numel() == 1 and dropout_key.is_cuda
        return [ops.DropOperands(dropout_key, k, drop_pass, self.drop_thr, self.drop_scale) for k in range(n)]

    def forward_nhwc(self, x, t, save: bool, refresh_weights: bool = True, classes=None, dropout_key=None, drop_pass: int = 0,
                     lowres_s=None):
        """x: [B, S, S, in_pitch] NHWC (``input_buffer``; pad lanes zero), t: int64 [B] - float32 [B], a real-valued time, on a
        network with the random / learned fourier embedding (``check_time``: the other type is a TypeError).
        Returns (out [B,S,S,r4(out_dim)], tape).  ``refresh_weights=False``: the derived weight copies (Winograd /
        split-precision operands) are known to be current — a sampling chain refreshes them once, not per step.
        ``classes``: int64 [B] on the device (``Unet.labels``), read by a class-conditional network only; None = null labels.
        ``dropout_key`` (int64 [1] on the device, read by the kernels when they run) / ``drop_pass``: the passes of the training
        loss hand them in - 0 the trained pass, 1 the self-conditioning estimate; a network with ``dropout > 0`` in training mode
        then drops.  Every other caller (samplers, likelihood, ``forward``) passes none and never drops.
        ``lowres_s``: int64 [B] on the device (``Unet.aug_levels``), the augmentation levels a low-resolution conditioned
        network embeds; its conditioning image is in the buffer's slice [cond_off, cond_off + C) already."""
        B, S, _, _ = x.shape
        t = self.check_time(t)
        dro = self.drop_operands(dropout_key, drop_pass)
        dim = self.dim
        n = len(self.in_out)
        assert S % (2 ** (n - 1)) == 0, f"input size {S} must be divisible by {2 ** (n - 1)}"
        if refresh_weights:
            self.refresh_derived_weights(save)
        ss_all, time_saved = self._time_fwd(t, save, classes, lowres_s)
        ssl = [ss_all[:, o:o + 2 * rb.dim_out] for o, rb in zip(self._ss_offsets, self.resblocks())]
        k = 0  # running resblock index
        tape = []
        # final concat buffer (x, r): r = init_conv output lives in its upper half
        catF = ops.new((B, S, S, 2 * dim), x)
        r = _chan(catF, dim, 2 * dim)
        self.init_conv.fwd(x, out=r)
        cur = r
        res = S
        cats = []
        for s, (b1, b2, attn, down) in enumerate(self.downs):
            ci, co = self.in_out[s]
            cat1 = ops.new((B, res, res, co + ci), x)   # (x_up, h_b)
            cat2 = ops.new((B, res, res, co + ci), x)   # (x_up', h_a)
            cats.append((cat1, cat2))
            ha = _chan(cat2, co, co + ci)
            hb = _chan(cat1, co, co + ci)
            s1 = b1.fwd(cur, ssl[k], ha, save, dro[k]); k += 1
            mid = ops.new((B, res, res, ci), x)
            s2 = b2.fwd(ha, ssl[k], mid, save, dro[k]); k += 1
            s3 = attn.fwd(mid, hb, save)
            last = s == n - 1
            nres = res if last else res // 2
            nxt = ops.new((B, nres, nres, co), x)
            s4 = down.fwd_s(hb, nxt, save) if last else down.fwd(hb, nxt, save)
            tape.append((s1, s2, s3, s4))
            cur, res = nxt, nres
        m1 = ops.new(cur.shape, x)
        sm1 = self.mid_block1.fwd(cur, ssl[k], m1, save, dro[k]); k += 1
        m2 = ops.new(cur.shape, x)
        sm2 = self.mid_attn.fwd(m1, m2, save)
        # mid_block2 writes straight into the first up-stage concat buffer
        ups_tape = []
        for u, (b1, b2, attn, up) in enumerate(self.ups):
            s = n - 1 - u
            ci, co = self.in_out[s]
            cat1, cat2 = cats[s]
            xa = _chan(cat1, 0, co)
            if u == 0:
                sm3 = self.mid_block2.fwd(m2, ssl[k], xa, save, dro[k]); k += 1
            # (for u > 0 the previous up-stage already wrote xa)
            xb = _chan(cat2, 0, co)
            s1 = b1.fwd(cat1, ssl[k], xb, save, dro[k]); k += 1
            y2 = ops.new((B, res, res, co), x)
            s2 = b2.fwd(cat2, ssl[k], y2, save, dro[k]); k += 1
            y3 = ops.new((B, res, res, co), x)
            s3 = attn.fwd(y2, y3, save)
            last = u == n - 1
            if last:
                dst = _chan(catF, 0, dim)
                s4 = up.fwd_s(y3, dst, save)
            else:
                ci_n, co_n = self.in_out[s - 1]
                dst = _chan(cats[s - 1][0], 0, co_n)
                s4 = up.fwd(y3, dst, save)
                res *= 2
            ups_tape.append((s1, s2, s3, s4))
        fin = ops.new((B, S, S, dim), x)
        sf = self.final_res_block.fwd(catF, ssl[k], fin, save, dro[k]); k += 1
        out = self.final_conv.fwd(fin)
        if not save:
            return out, None
        return out, NetworkTape(time_saved, tape, sm1, sm2, sm3, ups_tape, sf, fin, x, [c[0].shape for c in cats])

    def refresh_derived_weights(self, for_backward: bool):
        if self._flat.b3:
            self._flat.refresh_split()      # bf16 planes of the current weights (one launch)
        if self._flat.wino:
            self._flat.refresh_wino(backward_operand=for_backward)   # U = G g G^T of the current weights (one launch)

    def backward_nhwc(self, tape: "NetworkTape", gout):
        """Hand-written backward pass: parameter gradients into the flat gradient buffer."""
        self.backward_run(self.backward_begin(tape, gout))

    def _flush(self, gc: GradCtx, bucket: int):
        """End of an exchange bucket (0: ups + final, 1: mid, 2: init + downs, 3: FiLM + time): the deferred slab / row
        reductions of its layers.  Normally ONE batched launch right here.  While a step is being captured with
        ``_flush_collect`` set (lgm_hip.graph.GraphedDDPMStep) the descriptor rows are handed to the step object
        instead, which launches the reduction - and the bucket's all-reduce and Adam slice behind it - on a side stream
        next to the following backward phase: weight-sized, HBM-bound passes beside MFMA-bound convolutions."""
        col = getattr(self, "_flush_collect", None)
        gc.finish_pending()              # a large-map weight gradient still waiting for a partner (GradCtx.queue_wgrad)
        if col is None:
            gc.flush()
        else:
            col[bucket] = list(gc.deferred or [])
            if gc.deferred is not None:
                gc.deferred.clear()

    def bucket_ranges(self):
        """Flat-buffer slices of the four exchange buckets, in backward completion order: bucket k is final when phase k
        of the backward pass (``BACKWARD_PHASES``) ends.  [ups] + [final] are 18.6 M of the 35.7 M parameters at dim 64,
        [mid] 10.2 M: their exchange overlaps everything that follows."""
        t = self._flat.total
        return [[(self._ups_start, self._mid_start), (self._final_start, t)], [(self._mid_start, self._final_start)],
                [(self._head_end, self._ups_start)], [(0, self._head_end)]]

    def _bucket_done(self, gc: GradCtx, bucket: int):
        """The last statement of phase ``bucket``: its reductions, then its slices go to the gradient exchange."""
        self._flush(gc, bucket)
        sync = getattr(self, "grad_sync", None)
        if sync is not None:
            for lo, hi in self.bucket_ranges()[bucket]:
                sync.ready(lo, hi)
        if bucket == 3:                  # the whole gradient buffer is final
            self._flat.bind_grad_views()

    def backward_begin(self, tape: "NetworkTape", gout):
        """The state the phases work on; no phase has run."""
        return _Backward(self, tape, gout)

    def backward_run(self, st: "_Backward", first: int = 0, last: int = 3):
        """Phases ``first`` .. ``last`` of the backward pass ``backward_begin`` opened."""
        for phase in self.BACKWARD_PHASES[first:last + 1]:
            phase(self, st)

    def _backward_up(self, st: "_Backward"):
        """final conv -> final block -> up path"""
        gc, gsl, k, x_in = st.gc, st.gsl, st.k, st.x_in
        ups_tape, sf, fin, cat_shapes, gout, held = st.ups, st.final, st.fin, st.cat_shapes, st.gout, st.held
        st.ups = st.final = st.fin = st.cat_shapes = st.gout = st.held = None
        B, S = x_in.shape[0], x_in.shape[1]
        dim = self.dim
        n = len(self.in_out)
        gfin = self.final_conv.bwd(gc, fin, gout)
        gcatF = ops.new((B, S, S, 2 * dim), x_in)
        self.final_res_block.bwd(gc, sf, gfin, gsl[k], gcatF, False); k -= 1
        del gfin
        gcats = [None] * n
        g_next = _chan(gcatF, 0, dim)     # grad of the last up-stage output
        for u in range(n - 1, -1, -1):
            b1, b2, attn, up = self.ups[u]
            s = n - 1 - u
            ci, co = self.in_out[s]
            s1, s2, s3, s4 = ups_tape[u]
            shp = cat_shapes[s]
            res = shp[1]
            gy3 = ops.new((B, res, res, co), x_in)
            if u == n - 1:
                up.bwd_s(gc, s4, g_next, gy3, False)
            else:
                up.bwd(gc, s4, g_next, gy3, False)
            gy2 = ops.new((B, res, res, co), x_in)
            attn.bwd(gc, s3, gy3, gy2, False)
            del gy3
            gcat2 = ops.new(shp, x_in)
            b2.bwd(gc, s2, gy2, gsl[k], gcat2, False); k -= 1
            del gy2
            gcat1 = ops.new(shp, x_in)
            b1.bwd(gc, s1, _chan(gcat2, 0, co), gsl[k], gcat1, False); k -= 1
            gcats[s] = (gcat1, gcat2)
            g_next = _chan(gcat1, 0, co)
        st.k, st.gcats, st.gcatF, st.g = k, gcats, gcatF, g_next
        self._bucket_done(gc, 0)

    def _backward_mid(self, st: "_Backward"):
        """middle blocks"""
        gc, gsl, k, g_next, x_in = st.gc, st.gsl, st.k, st.g, st.x_in
        sm1, sm2, sm3 = st.mid
        gm2 = ops.new(sm3[0].shape, x_in)
        self.mid_block2.bwd(gc, sm3, g_next, gsl[k], gm2, False); k -= 1
        gm1 = ops.new(gm2.shape, x_in)
        self.mid_attn.bwd(gc, sm2, gm2, gm1, False)
        del gm2
        gcur = ops.new(gm1.shape, x_in)
        self.mid_block1.bwd(gc, sm1, gm1, gsl[k], gcur, False); k -= 1
        del gm1
        st.k, st.g = k, gcur
        self._bucket_done(gc, 1)

    def _backward_down(self, st: "_Backward"):
        """down path -> init conv"""
        gc, tape, gsl, k, gcats, gcatF, gcur, x_in = st.gc, st.tape, st.gsl, st.k, st.gcats, st.gcatF, st.g, st.x_in
        dim = self.dim
        n = len(self.in_out)
        for s in range(n - 1, -1, -1):
            b1, b2, attn, down = self.downs[s]
            ci, co = self.in_out[s]
            s1, s2, s3, s4 = tape[s]
            gcat1, gcat2 = gcats[s]
            ghb = _chan(gcat1, co, co + ci)   # already holds the skip-connection gradient
            gha = _chan(gcat2, co, co + ci)
            if s == n - 1:
                down.bwd_s(gc, s4, gcur, ghb, True)
            else:
                down.bwd(gc, s4, gcur, ghb, True)
            gmid = ops.new(s3[0].shape, x_in)
            attn.bwd(gc, s3, ghb, gmid, False)
            b2.bwd(gc, s2, gmid, gsl[k], gha, True); k -= 1
            del gmid
            if s == 0:
                gr = _chan(gcatF, dim, 2 * dim)   # init_conv output also feeds the final concat
                b1.bwd(gc, s1, gha, gsl[k], gr, True); k -= 1
                gcur = gr
            else:
                gprev = ops.new(s1[0].shape, x_in)
                b1.bwd(gc, s1, gha, gsl[k], gprev, False); k -= 1
                gcur = gprev
        assert k == -1
        self.init_conv.bwd(gc, x_in, gcur, need_gx=False)
        self._bucket_done(gc, 2)

    def _backward_time(self, st: "_Backward"):
        """time embedding / FiLM projections"""
        self._time_bwd(st.gc, st.time_saved, st.gss_all)
        self._bucket_done(st.gc, 3)

    BACKWARD_PHASES = (_backward_up, _backward_mid, _backward_down, _backward_time)

    def forward(self, x: torch.Tensor, time: torch.Tensor, x_self_cond=None, classes=None, lowres_cond_img=None,
                lowres_aug_t=None) -> torch.Tensor:
        """NCHW in / NCHW out, like the reference Unet.forward (:428-471); ``x_self_cond`` is a constant (no gradient
        reaches it) and is read by a self-conditioned network only, ``None`` meaning zeros (:434).  ``classes`` (extension):
        one label in [0, num_classes] per sample for a class-conditional network, ``None`` meaning the null label; on a
        network without classes it raises ValueError.  ``lowres_cond_img`` / ``lowres_aug_t`` (extension): the conditioning
        image of a low-resolution conditioned network, already at x's size and in x's range (a constant: no gradient reaches
        it), and its augmentation levels (``None`` = 0); the image is required there and a ValueError on any other network."""
        time = self.check_time(time)       # here too: the refusal comes before any storage is bound (forward_nhwc serves the samplers)
        classes = self.labels(classes, x.shape[0], x.device)
        if self.lowres_cond:
            if lowres_cond_img is None:
                raise ValueError("a Unet built with lowres_cond=True needs lowres_cond_img")
            if tuple(lowres_cond_img.shape) != tuple(x.shape):
                raise ValueError(f"lowres_cond_img {tuple(lowres_cond_img.shape)} must have the shape of x {tuple(x.shape)}")
        elif lowres_cond_img is not None:
            raise ValueError("lowres_cond_img was passed to a Unet built without lowres_cond")
        s = self.aug_levels(lowres_aug_t, x.shape[0], x.device)
        return _UnetFn.apply(self._anchor(x.device), self, x, time, x_self_cond, classes, lowres_cond_img, s)

    # ---- the input buffer and its two slices ------------------------------------------------------------
    def input_buffer(self, B, H, W, like):
        return ops.new((B, H, W, self.in_pitch), like)

    def x_slice(self, xin, pad: bool = False):
        """The lanes of ``x`` in an input buffer; ``pad``: and the padding behind them (a producer that zero-fills it)."""
        return _chan(xin, self.x_off, self.in_pitch if pad else self.x_off + self.channels)

    def sc_slice(self, xin):
        return _chan(xin, self.sc_off, self.sc_off + self.channels)

    def cond_slice(self, xin):
        """the lanes of the low-resolution conditioning image"""
        return _chan(xin, self.cond_off, self.cond_off + self.channels)

    def x_extent(self):
        """(first lane, lanes) the kernels that rewrite x own in an input buffer of a low-resolution conditioned network"""
        return self.x_off, self.in_pitch - self.x_off

    def _anchor(self, device):
        self.prepare_hip(device)
        a = getattr(self, "_anchor_t", None)
        if a is None or a.device != torch.device(device):
            a = torch.zeros(1, device=device, requires_grad=True)
            self._anchor_t = a
        return a

    def run_nchw(self, x, time, save, x_self_cond=None, classes=None, cond_scale: float = 1.0, lowres_cond_img=None,
                 lowres_s=None):
        """``classes``: device labels (``Unet.labels``); ``cond_scale != 1`` (without saved activations only): guided output"""
        B, C, H, W = x.shape
        xin = self.input_buffer(B, H, W, x)
        ops.nchw_to_nhwc(x.contiguous(), self.x_slice(xin, pad=True))
        if self.self_condition:
            sc = torch.zeros_like(x) if x_self_cond is None else x_self_cond.detach().float().contiguous()
            assert sc.shape == x.shape, f"x_self_cond {tuple(sc.shape)} must have the shape of x {tuple(x.shape)}"
            ops.nchw_to_nhwc(sc, self.sc_slice(xin))
        if self.lowres_cond:
            ops.nchw_to_nhwc(lowres_cond_img.detach().float().contiguous(), self.cond_slice(xin))
        if save:
            assert float(cond_scale) == 1.0, "guidance is a sampling-time mix: no gradient is taken through it"
            out, tape = self.forward_nhwc(xin, time, True, True, classes, lowres_s=lowres_s)
        else:
            out, tape = self.forward_guided(xin, time, classes, cond_scale, lowres_s=lowres_s), None
        y = ops.new((B, self.out_dim, H, W), x)
        ops.nhwc_to_nchw(out, y)
        return y, tape, out


# What ``Unet.forward_nhwc(save=True)`` keeps for the backward pass: per stage of ``downs`` / ``ups`` what its two blocks, its
# attention and its resampling saved, ``sm1`` .. ``sm3`` the middle blocks', ``final`` / ``fin`` the final block's and its output.
NetworkTape = namedtuple("NetworkTape", ["time_saved", "downs", "sm1", "sm2", "sm3", "ups", "final", "fin", "x", "cat_shapes"])
# ``time_saved``, what ``Unet._time_fwd(save=True)`` keeps: the time MLP's activations, the embedding sum and its SiLU, the labels
# (None without classes) and ``lowres`` = (pe_s, a1_s, h_s) of ``lowres_time_mlp`` (None without low-resolution conditioning).
TimeTape = namedtuple("TimeTape", ["pe", "a1", "h", "temb", "st", "classes", "lowres"])


class _Backward:
    """What the phases of ``Unet``'s backward pass hand to each other: the gradient context, the saved activations the
    later phases read, the gradients of the FiLM projections (``gss_all``, ``gsl`` its per-block views), the running
    resblock index ``k``, the gradient concat buffers (``gcats``, ``gcatF``), the current gradient ``g`` and the
    network input.  ``ups`` / ``final`` / ``fin`` / ``cat_shapes`` / ``gout``: what the first phase alone reads; ``held``: what
    else is to live until that phase returns (callers append).  It takes them all out of here before it starts."""

    def __init__(self, net: Unet, tape: NetworkTape, gout):
        x_in = tape.x
        rbs = net.resblocks()
        self.gc = GradCtx(net._flat, defer=True)     # weight-gradient slabs: one batched reduce per exchange bucket
        self.time_saved, self.tape, self.mid, self.x_in = tape.time_saved, tape.downs, (tape.sm1, tape.sm2, tape.sm3), x_in
        self.ups, self.final, self.fin, self.cat_shapes, self.gout = tape.ups, tape.final, tape.fin, tape.cat_shapes, gout
        self.held = []
        self.gss_all = ops.new((x_in.shape[0], net._ss_total), x_in)
        self.gsl = [self.gss_all[:, o:o + 2 * rb.dim_out] for o, rb in zip(net._ss_offsets, rbs)]
        self.k = len(rbs) - 1
        self.gcats = self.gcatF = self.g = None


class _UnetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, net: Unet, x, time, x_self_cond=None, classes=None, lowres_cond_img=None, lowres_s=None):
        save = bool(ctx.needs_input_grad[0])   # grad mode on at apply() time and anchor requires grad
        y, tape, _ = net.run_nchw(x.detach().float(), time, save, x_self_cond, classes, 1.0, lowres_cond_img, lowres_s)
        ctx.net, ctx.tape = net, tape
        return y

    @staticmethod
    def backward(ctx, gy):
        net, tape = ctx.net, ctx.tape
        if tape is None:
            raise RuntimeError("Unet forward ran without saving activations")
        B, C, H, W = gy.shape
        g = ops.new((B, H, W, _r4(C)), gy)
        ops.nchw_to_nhwc(gy.contiguous(), g)
        net.backward_nhwc(tape, g)
        ctx.tape = None
        return None, None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------
# Gaussian diffusion  (reference :532-946)
# ----------------------------------------------------------------------------------------
def _sigmoid_beta_schedule(timesteps, start=-3, end=3, tau=1):
    t = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64) / timesteps
    v0 = torch.tensor(start / tau).sigmoid()
    v1 = torch.tensor(end / tau).sigmoid()
    ac = (v1 - ((t * (end - start) + start) / tau).sigmoid()) / (v1 - v0)
    ac = ac / ac[0]
    return torch.clip(1 - ac[1:] / ac[:-1], 0, 0.999)


def _linear_beta_schedule(timesteps):
    scale = 1000 / timesteps
    return torch.linspace(scale * 0.0001, scale * 0.02, timesteps, dtype=torch.float64)


def _cosine_beta_schedule(timesteps, s=0.008):
    t = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64) / timesteps
    ac = torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - ac[1:] / ac[:-1], 0, 0.999)


OBJECTIVES = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}     # the `objective` argument of the lgm_*_obj entry points


class _Distillation:
    """What ``GaussianDiffusion.distill_from`` attaches: the frozen teacher network (``teacher``, a ``Unet`` of its own flat
    storage - deliberately no submodule of the student), the teacher's objective, the clip flag, and for the student's step
    count ``steps``: ``grid`` (the host list G), ``levels`` (int64 [N], G[:-1] on the device: t = levels[i]) and ``table``
    (float32 [T, 16], ``lgm_hip.distill.distill_plan`` rounded once).  ``stale``: the teacher's derived weight copies (Winograd
    operands) are to be refreshed by its next forward - set whenever its weights may have changed, never inside a replay."""

    def __init__(self, teacher: Unet, objective: str, clip: bool):
        self.teacher, self.objective, self.clip = teacher, objective, clip
        self.steps, self.grid, self.levels, self.table, self.stale = None, None, None, None, True

    def plan(self, gd: "GaussianDiffusion", steps: int):
        from lgm_hip import distill
        rows = distill.distill_plan(gd, steps)
        self.steps, self.grid = int(steps), distill.distill_grid(gd.num_timesteps, steps)[0]
        self.levels = torch.tensor(self.grid[:-1], dtype=torch.long, device=gd.device)
        self.table = rows.to(torch.float32).to(gd.device).contiguous()

    def apply(self, fn):
        self.teacher._apply(fn)
        self.levels, self.table, self.stale = fn(self.levels), fn(self.table), True

    def load_teacher(self, state):
        self.teacher.load_state_dict(state, strict=True)
        fp = self.teacher._flat
        if fp is not None and fp.device.type == "cuda" and fp.still_bound():
            self.teacher.refresh_derived_weights(False)      # now: a captured step does not pass through Python again
            self.stale = False
        else:
            self.stale = True


class Diffusion(nn.Module):
    """What ``GaussianDiffusion`` and ``ElucidatedDiffusion`` (edm.py) share, and the protocol of the training step - eager
    (``forward`` / ``p_losses``) and graph-replayed (``lgm_hip.graph.GraphedDDPMStep``) alike: a diffusion defines
    ``draw(x, labels, ...) -> StepDraws``, the ONE place its draw order is written, and ``qsample(x, draws, normalize) ->
    QSample``, its launches up to the network's input buffer and the target.  Everything behind them (``hip_loss_network``)
    reads ``model``, ``auto_normalize``, ``loss_weight`` and what stands below.  Registers no parameter, buffer or submodule."""
    learned_variance = False                         # hip_loss_network: the hybrid loss
    _distill = None                                  # DDPMFastStep.step, DDPM.prepare_hip: the attached teacher

    @property
    def device(self):
        return self.loss_weight.device

    def active_t_sampler(self):
        """the timestep sampler a forward in the current mode goes through (``lgm_hip.tsampler``), or None"""
        return None

    def draw_dropout_key(self, device):
        """The step's 64-bit dropout key: ONE persistent int64 [1] device tensor, refilled in place from torch's device
        generator (one launch; capturable).  The kernels read it when they run, so the backward pass sees the key of its
        forward as long as no other loss forward of this diffusion runs in between.  None when the loss passes do not drop
        (``dropout == 0`` or evaluation mode): nothing is drawn, nothing allocated."""
        if self.model.dropout <= 0.0 or not self.model.training:
            return None
        key = self.__dict__.get("dropout_key")
        if key is None or key.device != torch.device(device):
            key = self.__dict__["dropout_key"] = torch.zeros(1, dtype=torch.int64, device=device)
        return key.random_(-2 ** 63, None)             # all 64 bits

    def drop_labels(self, classes):
        """Classifier-free guidance training: every label becomes the null label with probability ``cond_drop_prob`` (one
        ``torch.rand(B)`` on the labels' device; nothing is drawn when the probability is 0)."""
        if self.cond_drop_prob <= 0.0:
            return classes
        drop = torch.rand(classes.shape[0], device=classes.device) < self.cond_drop_prob
        return torch.where(drop, torch.full_like(classes, self.num_classes), classes)

    def step_labels(self, labels, classes, B, device):
        """The labels the network gets: the batch's ``labels`` behind the label drop (drawn here), or - no labels given -
        ``classes`` as they are (``Unet.labels``: None on a class-conditional network = the null label, nothing is drawn)."""
        if labels is None:
            return self.model.labels(classes, B, device)
        return self.drop_labels(self.model.labels(labels, B, device))

    def normalize(self, img):
        return img * 2 - 1 if self.auto_normalize else img

    def unnormalize(self, t):
        return (t + 1) * 0.5 if self.auto_normalize else t

    def _loss(self, img, loss_forward):
        """``loss_forward(save) -> (loss[1], LossContext)`` under the hand-written backward"""
        return _LossFn.apply(self.model._anchor(img.device), loss_forward)


class GaussianDiffusion(Diffusion):
    def __init__(self, model: Unet, *, img_size, timesteps=1000, sampling_timesteps=None, objective="pred_v",
                 beta_schedule="sigmoid", schedule_fn_kwargs=None, ddim_sampling_eta=0.0, auto_normalize=True,
                 offset_noise_strength=0.0, min_snr_loss_weight=False, min_snr_gamma=5, cond_drop_prob=None,
                 cond_scale=1.0, sampler="auto", dpm_order=2, dpm_stochastic=False, dynamic_thresholding=False,
                 dynamic_thresholding_percentile=0.995, vb_loss_weight=None, t_sampler="uniform", t_sampler_history=10,
                 t_sampler_uniform_prob=0.001, lowres_factor=4, lowres_aug_levels=None, lowres_sample_aug_t=None):
        """``lowres_factor`` / ``lowres_aug_levels`` / ``lowres_sample_aug_t`` (extension, read with a ``Unet(lowres_cond=True)``
        only - a super-resolution stage of a cascade): the stage conditions on its input area-averaged over ``lowres_factor`` x
        ``lowres_factor`` blocks (2, 4 or 8), upsampled bilinearly back and noise-augmented (Ho et al. 2021, conditioning
        augmentation) - c = sqrt_ac[s] u + sqrt_1mac[s] eps with s ~ randint(0, ``lowres_aug_levels``) per sample in training
        (``None`` = every level, as in Imagen) and s = ``lowres_sample_aug_t`` (``None`` = int(0.2 T)) in ``sample``.
        ``cond_drop_prob`` / ``cond_scale`` (extension, class-conditional ``model`` only): the probability with which
        ``forward`` replaces a training label by the null label, and the classifier-free-guidance scale ``sample`` uses.
        ``cond_drop_prob=None`` is 0.1 on a class-conditional model and 0 on any other.
        ``sampler`` (extension): ``"auto"`` = the reference's dispatch (DDIM when ``sampling_timesteps < timesteps``, else the
        ancestral chain), ``"dpm++"`` = DPM-Solver++ in ``sampling_timesteps`` steps of order ``dpm_order`` (2 = the 2M
        multistep, 1 = DDIM at eta 0), ``dpm_stochastic`` its SDE form.
        ``dynamic_thresholding`` (extension; Saharia et al. 2022, 2.3): wherever sampling clips x0 to [-1, 1] it computes
        ``s = max(1, quantile_p(|x0|))`` per sample instead, p = ``dynamic_thresholding_percentile`` in (0, 1], and takes
        ``clamp(x0, -s, s) / s``.  Training is untouched.
        ``vb_loss_weight`` (extension; Nichol & Dhariwal 2021, L_hybrid; a ``Unet(learned_variance=True)`` only, ``None`` =
        0.001 there): the model trains on mean_b(loss_weight[t_b] mse_b) + vb_loss_weight mean_b(vb_b), vb_b the bound's term at
        t_b in bits per dimension with the model mean detached; the ancestral chain samples with the learned variance and
        ``vlb_terms(variance="learned")`` evaluates the bound with it.  DDIM and DPM-Solver++ read no model variance.
        ``t_sampler`` (extension): how a TRAINING-mode forward draws t.  ``"uniform"``: the reference's ``randint``.
        ``"stratified"``: one uniform per step, t_b = floor(T (u0 + b / B mod 1)) (Kingma et al. 2021, VDM App. I.1).
        ``"loss_second_moment"`` (Nichol & Dhariwal 2021, 3.3): p_t proportional to the root mean square of the last
        ``t_sampler_history`` per-sample losses seen at t, mixed with ``t_sampler_uniform_prob`` of the uniform distribution
        once every t has a full history, and the loss is mean_b(L_b / (T p_t_b)), which leaves its gradient unbiased
        (``lgm_hip.tsampler``; ``p_losses`` with an explicit t weights and records the same way).  In eval mode every sampler
        draws uniformly, weights nothing and records nothing.  A deep copy (the EMA shadow) is a ``"uniform"`` diffusion: the
        state lives with the model that trains, under ``t_sampler.history`` / ``t_sampler.counts`` of its state dict."""
        super().__init__()
        from lgm_hip import tsampler
        if getattr(model, "random_or_learned_sinusoidal_cond", False):       # the reference asserts the same (:555)
            raise ValueError("GaussianDiffusion walks integer timesteps: a Unet with the random / learned fourier embedding "
                             "reads a real-valued time (models.generative.diffusion.edm.ElucidatedDiffusion)")
        history, uniform_prob = tsampler.check_arguments(t_sampler, t_sampler_history, t_sampler_uniform_prob)
        self.t_sampler = t_sampler
        self.learned_variance = bool(getattr(model, "learned_variance", False))
        if vb_loss_weight is not None and not self.learned_variance:
            raise ValueError("vb_loss_weight needs a model built with learned_variance=True")
        if self.learned_variance and model.out_dim != 2 * model.channels:
            raise ValueError(f"a learned-variance model has out_dim = 2 * channels, got {model.out_dim}")
        vb_loss_weight = 0.001 if vb_loss_weight is None else float(vb_loss_weight)
        if not vb_loss_weight >= 0.0:
            raise ValueError(f"vb_loss_weight must not be negative, got {vb_loss_weight!r}")
        self.vb_loss_weight = vb_loss_weight
        p = dynamic_thresholding_percentile
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 < float(p) <= 1.0:
            raise ValueError(f"dynamic_thresholding_percentile must lie in (0, 1], got {p!r}")
        self.dynamic_thresholding, self.dynamic_thresholding_percentile = bool(dynamic_thresholding), float(p)
        if sampler not in ("auto", "dpm++"):
            raise ValueError(f"sampler must be 'auto' or 'dpm++', got {sampler!r}")
        if dpm_order not in (1, 2):
            raise ValueError(f"dpm_order must be 1 or 2, got {dpm_order!r}")
        if sampler == "dpm++" and sampling_timesteps is None:
            raise ValueError("sampler='dpm++' needs sampling_timesteps (the number of solver steps)")
        self.sampler, self.dpm_order, self.dpm_stochastic = sampler, int(dpm_order), bool(dpm_stochastic)
        if objective not in OBJECTIVES:
            raise ValueError(f"objective must be one of {sorted(OBJECTIVES)}, got {objective!r}")
        self.num_classes = getattr(model, "num_classes", None)
        if cond_drop_prob is None:
            cond_drop_prob = 0.1 if self.num_classes is not None else 0.0
        if not 0.0 <= float(cond_drop_prob) <= 1.0:
            raise ValueError(f"cond_drop_prob must lie in [0, 1], got {cond_drop_prob!r}")
        if self.num_classes is None and (float(cond_drop_prob) > 0.0 or float(cond_scale) != 1.0):
            raise ValueError("cond_drop_prob > 0 and cond_scale != 1 need a model built with num_classes")
        self.cond_drop_prob, self.cond_scale = float(cond_drop_prob), float(cond_scale)
        self.model = model
        self.channels = model.channels
        self.self_condition = model.self_condition
        self.img_size = img_size
        self.lowres_cond = bool(getattr(model, "lowres_cond", False))
        self.lowres_factor = int(lowres_factor)
        if self.lowres_cond:
            if self.lowres_factor not in ops.LOWRES_FACTORS:
                raise ValueError(f"lowres_factor must be one of {ops.LOWRES_FACTORS}, got {lowres_factor!r}")
            if int(img_size) % self.lowres_factor:
                raise ValueError(f"lowres_factor {self.lowres_factor} does not divide img_size {img_size}")
        self.objective = objective
        self.offset_noise_strength = offset_noise_strength
        fn = {"linear": _linear_beta_schedule, "cosine": _cosine_beta_schedule, "sigmoid": _sigmoid_beta_schedule}
        if beta_schedule not in fn:
            raise ValueError(f"unknown beta schedule {beta_schedule}")
        betas = fn[beta_schedule](timesteps, **(schedule_fn_kwargs or {}))
        alphas = 1.0 - betas
        ac = torch.cumprod(alphas, dim=0)
        ac_prev = torch.nn.functional.pad(ac[:-1], (1, 0), value=1.0)
        self.num_timesteps = int(betas.shape[0])
        levels = self.num_timesteps if lowres_aug_levels is None else int(lowres_aug_levels)
        sample_s = int(0.2 * self.num_timesteps) if lowres_sample_aug_t is None else int(lowres_sample_aug_t)
        if self.lowres_cond and not (1 <= levels <= self.num_timesteps and 0 <= sample_s < self.num_timesteps):
            raise ValueError(f"lowres_aug_levels must lie in [1, {self.num_timesteps}] and lowres_sample_aug_t in "
                             f"[0, {self.num_timesteps}), got {lowres_aug_levels!r} and {lowres_sample_aug_t!r}")
        self.lowres_aug_levels, self.lowres_sample_aug_t = levels, sample_s
        self.sampling_timesteps = sampling_timesteps if sampling_timesteps is not None else self.num_timesteps
        assert self.sampling_timesteps <= self.num_timesteps
        self.is_ddim_sampling = self.sampling_timesteps < self.num_timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
        snr = ac / (1 - ac)
        clipped = snr.clone()
        if min_snr_loss_weight:
            clipped.clamp_(max=min_snr_gamma)
        reg = lambda n, v: self.register_buffer(n, v.to(torch.float32))  # noqa: E731
        reg("betas", betas)
        reg("alphas_cumprod", ac)
        reg("alphas_cumprod_prev", ac_prev)
        reg("sqrt_alphas_cumprod", torch.sqrt(ac))
        reg("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - ac))
        reg("log_one_minus_alphas_cumprod", torch.log(1.0 - ac))
        reg("sqrt_recip_alphas_cumprod", torch.sqrt(1.0 / ac))
        reg("sqrt_recipm1_alphas_cumprod", torch.sqrt(1.0 / ac - 1))
        reg("posterior_variance", post_var)
        reg("posterior_log_variance_clipped", torch.log(post_var.clamp(min=1e-20)))
        reg("posterior_mean_coef1", betas * torch.sqrt(ac_prev) / (1.0 - ac))
        reg("posterior_mean_coef2", (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac))
        reg("loss_weight", {"pred_noise": clipped / snr, "pred_x0": clipped, "pred_v": clipped / (snr + 1)}[objective])
        self.auto_normalize = auto_normalize
        if self.learned_variance:
            # the per-t scalars of the hybrid loss, [T, 8] = (log beta_t, log beta~_t, lv_q, P1, P2, 0, 0, 0): float64 from the
            # tables above, rounded once (lgm_hip.likelihood.learned_table); not part of any state dict
            from lgm_hip.likelihood import learned_table
            self.register_buffer("learned_table", torch.tensor(learned_table(self), dtype=torch.float32), persistent=False)
        # a plain attribute, not a submodule and not buffers: see lgm_hip.tsampler
        self._ts = None if t_sampler == "uniform" else tsampler.TimestepSampler(t_sampler, self.num_timesteps, history,
                                                                                uniform_prob)
        # progressive distillation (``distill_from``): None, or the attached teacher - a plain attribute like ``_ts``
        self._distill: Optional[_Distillation] = None

    # -- progressive distillation (extension; Salimans & Ho 2022, Algorithm 2; lgm_hip/distill.py) ------------------
    def distill_from(self, teacher: Optional["GaussianDiffusion"], steps: Optional[int] = None, clip: bool = True):
        """Attach a frozen copy of ``teacher.model``: from now on the training-mode ``forward`` / ``p_losses``, the eval-mode loss
        and the graph-replayed step train THIS model so that one of its DDIM steps on the ``steps``-step grid lands where two
        DDIM steps of the teacher on the 2 ``steps``-step grid land (module text of lgm_hip/distill.py).  The loss draws
        i ~ randint(0, steps) where randint(0, T) stood and t = G[i]; behind the q_sample launch come the teacher's forward at
        (z_t, t) without saved activations, ``lgm_distill_half_step``, its forward at (z_t', t') and ``lgm_distill_target``,
        whose output takes the place of the objective's target; the weighted MSE with this model's ``loss_weight[t]`` and
        everything behind it are unchanged.  ``clip`` (default True): the teacher's x0 predictions are clamped to [-1, 1] as
        ``ddim_sample`` clamps them.  A class-conditional teacher sees the labels the student sees (after the drop), unguided.
        Sets ``sampling_timesteps = steps``, DDIM sampling at eta 0 and ``sampler = "auto"``: ``sample()`` is the distilled sampler.
        The copy has its own flat storage, is in eval mode, needs no gradient and never drops; its weights are no parameters of
        this model (not in its flat buffer, gradient, optimizer or EMA shadow) and are saved and loaded under
        ``distill_teacher.*`` with ``distill_steps`` while attached.  A deep copy of this model carries no teacher.
        ``distill_from(None)`` detaches (the sampling settings stay).
        Refused: ``NotImplementedError`` for a student with ``self_condition``, ``learned_variance``, ``lowres_cond``,
        ``dropout > 0``, ``offset_noise_strength > 0`` or ``t_sampler != "uniform"`` and for a teacher with one of the first
        three; ``ValueError`` for a teacher whose channels, image size, schedule tables or ``num_classes`` differ, for
        ``2 * steps > T``, for a (T, steps) whose grids do not nest, and for ``sampler="dpm++"`` on the student."""
        from lgm_hip import distill
        if teacher is None:
            self._distill = None
            return self
        import copy
        N = distill.check_arguments(self, teacher, steps)
        net = copy.deepcopy(teacher.model)           # Unet.__deepcopy__: plain parameters, flat storage of its own
        net.eval().requires_grad_(False)
        net.dropout = 0.0
        self._distill = _Distillation(net, teacher.objective, bool(clip))
        self._distill.plan(self, N)
        self.set_sampling_steps(N)
        return self

    def set_sampling_steps(self, steps: int):
        """what ``distill_from`` sets on the student (and ``DDPM`` on its EMA shadow): ``sample()`` = DDIM in ``steps`` steps, eta 0"""
        self.sampling_timesteps = int(steps)
        self.is_ddim_sampling = self.sampling_timesteps < self.num_timesteps
        self.ddim_sampling_eta, self.sampler = 0.0, "auto"

    @property
    def distill_steps(self) -> Optional[int]:
        """N while a teacher is attached, else None"""
        return None if self._distill is None else self._distill.steps

    # -- the timestep sampler's state: moved, saved and loaded with the module, never a buffer of it ----------------
    def active_t_sampler(self):
        """the sampler a forward in the current mode goes through: None in eval mode and for ``"uniform"``"""
        return self._ts if self.training else None

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k in ("_ts", "_distill") else copy.deepcopy(v, memo)      # (no teacher either)
        new.t_sampler = "uniform"
        return new

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self._ts is not None:
            self._ts.apply(fn)
        if self._distill is not None:
            self._distill.apply(fn)
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self._ts is not None:
            for k, v in self._ts.state().items():
                destination[f"{prefix}t_sampler.{k}"] = v if keep_vars else v.detach()
        if self._distill is not None:
            for k, v in self._distill.teacher.state_dict().items():
                destination[f"{prefix}distill_teacher.{k}"] = v
            destination[f"{prefix}distill_steps"] = torch.tensor(self._distill.steps)

    def _load_distillation(self, state_dict, prefix, missing_keys, error_msgs):
        """With a teacher attached: its weights and the step count out of ``state_dict`` -> the dict without them.  A saved
        step count other than the attached one re-plans the grid and the table for it (a checkpoint of a later round)."""
        d, tp, sk = self._distill, f"{prefix}distill_teacher.", f"{prefix}distill_steps"
        if d is None:
            return state_dict
        found = {k[len(tp):]: v for k, v in state_dict.items() if k.startswith(tp)}
        rest = {k: v for k, v in state_dict.items() if not k.startswith(tp) and k != sk}
        if not found or sk not in state_dict:
            if sk not in state_dict:
                missing_keys.append(sk)
            if not found:
                missing_keys.extend(tp + k for k in d.teacher.state_dict())
            return rest
        try:
            d.load_teacher(found)
            steps = int(state_dict[sk])
            if steps != d.steps:
                d.plan(self, steps)
                self.set_sampling_steps(steps)
        except (RuntimeError, ValueError) as e:
            error_msgs.append(f"distill_teacher: {e}")
        return rest

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict = self._load_distillation(state_dict, prefix, missing_keys, error_msgs)
        mine = {k: f"{prefix}t_sampler.{k}" for k in (self._ts.state() if self._ts is not None else {})}
        found = {k: state_dict[key] for k, key in mine.items() if key in state_dict}
        rest = {k: v for k, v in state_dict.items() if k not in mine.values()} if found else state_dict
        super()._load_from_state_dict(rest, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if len(found) == len(mine) and mine:
            try:
                self._ts.load_state(found["history"], found["counts"])
            except ValueError as e:
                error_msgs.append(str(e))
        else:
            missing_keys.extend(key for k, key in mine.items() if k not in found)

    def ddim_time_pairs(self, steps=None):
        """the reference's DDIM grid (:785-787) on ``steps`` steps (default: ``sampling_timesteps``)"""
        times = torch.linspace(-1, self.num_timesteps - 1, steps=(self.sampling_timesteps if steps is None else steps) + 1)
        times = list(reversed(times.int().tolist()))
        return list(zip(times[:-1], times[1:]))

    def dpm_time_pairs(self):
        """the (t, t_next) grid of ``dpm_solver_sample``: the reference's DDIM grid, the last pair (t, -1) returning x0"""
        return self.ddim_time_pairs()

    # -- training ---------------------------------------------------------------------------
    def draw(self, x_start, labels=None, *, t=None, noise=None, offset=None, classes=None, dropout_key=None, lowres_aug_t=None,
             lowres_noise=None, offset_noise_strength=None) -> StepDraws:
        """The random operands of a training step on the batch ``x_start``: what is given is used, the rest is drawn from
        torch's device generator in THIS order, and nothing is drawn for a feature the diffusion does not have -
        t (a level of the student's grid under a teacher, the timestep sampler's draw in training mode, else randint),
        noise, the offset noise (strength > 0 only; ``offset_noise_strength`` overrides the attribute), the label drop
        (``labels`` given and ``cond_drop_prob > 0``; ``classes``: the labels as the network gets them, never dropped), the
        dropout key (``dropout > 0`` in training mode), the low-resolution level and noise (conditioned model)."""
        B, dev = x_start.shape[0], x_start.device
        if t is None:
            ts = self.active_t_sampler()
            if self._distill is not None:            # a level of the student's grid, where randint(0, T) stands
                t = self.draw_distill_t(B, dev)
            elif ts is None:
                t = torch.randint(0, self.num_timesteps, (B,), device=dev).long()
            else:                                    # (its uniforms stand where randint stands in the draw order)
                t = ts.draw(B, dev)
        if noise is None:
            noise = torch.randn_like(x_start)
        if not self._strength(offset_noise_strength) > 0.0:
            offset = None
        elif offset is None:
            offset = torch.randn(x_start.shape[:2], device=dev)
        classes = self.step_labels(labels, classes, B, dev)
        key = dropout_key if dropout_key is not None else self.draw_dropout_key(dev)
        return StepDraws(t, noise, offset, classes, key, self.draw_lowres(x_start, lowres_aug_t, lowres_noise))

    def qsample(self, x_start, d: StepDraws, normalize: bool, offset_noise_strength=None) -> QSample:
        """x_t, the objective's target and the conditioning slice from the batch and its draws (``hip_loss_qsample``); under a
        teacher the distillation target over the objective's (``hip_loss_distill``)."""
        q = hip_loss_qsample(self, x_start, d.t, d.noise, normalize, d.offset, self._strength(offset_noise_strength), d.lowres)
        if self._distill is not None:
            hip_loss_distill(self, q, d.classes)
        return q

    def _strength(self, offset_noise_strength=None):
        return self.offset_noise_strength if offset_noise_strength is None else offset_noise_strength

    def p_losses(self, x_start, t, noise=None, offset_noise_strength=None, classes=None, *, _offset_noise=None,
                 _normalize=False, _self_cond=None, _dropout_key=None, lowres_aug_t=None, lowres_noise=None,
                 _t_on_grid=False):
        """x_start already normalised unless _normalize (reference :878-925).  Offset noise (:885-891): one draw per
        (sample, channel), added to the noise inside the q_sample kernel - the caller's ``noise`` is not written.
        ``_offset_noise`` (extension, for parity tests): the [B, C] draw the reference takes from torch.randn.
        Self-conditioned model (:899-909): with probability 0.5 (Python's ``random.random()``, as in the reference) the network
        runs once without saved activations, its unclipped x_start becomes the self-conditioning input of the pass the
        gradient is taken through; no gradient reaches the estimate.  ``_self_cond`` (extension, for parity tests):
        ``True`` / ``False`` is the coin, an NCHW tensor is used as the estimate itself.
        ``classes`` (extension, class-conditional model): the labels as the network gets them - ``forward`` has already
        replaced the dropped ones by the null label; the estimate pass and the main pass see the same labels.
        Dropout (extension, ``Unet(dropout=p)`` in training mode): the step's key is drawn here behind every other draw (t,
        noise, offset noise, label drop); ``_dropout_key`` (for parity tests, like ``_offset_noise``): an int64 [1] device
        tensor used as the key instead, nothing is drawn.
        Low-resolution conditioned model (extension): the conditioning slice is made from ``x_start`` itself in one launch
        (``lgm_lowres_cond``); its augmentation level s ~ randint(0, lowres_aug_levels) per sample and its noise are drawn
        behind every other draw, so a model without the option draws what it drew; ``lowres_aug_t`` (int64 [B]) /
        ``lowres_noise`` (NCHW) are used instead when given (parity runs).
        With a teacher attached (``distill_from``): the target is the distillation target and every ``t_b`` must be a level
        of the student's grid that has a successor, G[:-1] - ValueError otherwise (``_t_on_grid``: ``forward`` drew them from
        the grid itself, nothing is read back).  Whatever is not given is drawn by ``draw``, in its order."""
        if self._distill is not None and not _t_on_grid:
            off = sorted(set(int(v) for v in t.tolist()) - set(self._distill.grid[:-1]))
            if off:
                raise ValueError(f"t = {off} is not on the student's {self._distill.steps}-step grid {self._distill.grid[:-1]}")
        if self._distill is not None and self._strength(offset_noise_strength) > 0.0:
            raise NotImplementedError("offset noise together with a distillation teacher is not built")
        d = self.draw(x_start, None, t=t, noise=noise, offset=_offset_noise, classes=classes, dropout_key=_dropout_key,
                      lowres_aug_t=lowres_aug_t, lowres_noise=lowres_noise, offset_noise_strength=offset_noise_strength)
        self_cond = False
        if self.self_condition:
            self_cond = (random.random() < 0.5) if _self_cond is None else _self_cond
        strength = float(self._strength(offset_noise_strength))
        return self._loss(x_start, lambda save: hip_loss_forward(self, x_start, d.t, d.noise, _normalize, save, d.offset,
                                                                 strength, self_cond, d.classes, d.dropout_key, d.lowres))

    def draw_lowres(self, x_start, lowres_aug_t=None, lowres_noise=None):
        """(s int64 [B], eps_aug like ``x_start``) of a training step on a low-resolution conditioned model - two draws from
        torch's device generator unless given -, None on any other model (nothing is drawn; given operands are a ValueError)."""
        if not self.lowres_cond:
            if lowres_aug_t is not None or lowres_noise is not None:
                raise ValueError("lowres_aug_t / lowres_noise were passed to a model built without lowres_cond")
            return None
        B = x_start.shape[0]
        if lowres_aug_t is None:
            s = torch.randint(0, self.lowres_aug_levels, (B,), device=x_start.device).long()
        else:
            s = self.model.aug_levels(lowres_aug_t, B, x_start.device)
        eps = torch.randn_like(x_start) if lowres_noise is None else lowres_noise
        return s, eps

    def draw_distill_t(self, B, device):
        """t of a distillation step: i ~ randint(0, N) from torch's device generator, t = G[i] by an index into the device copy of
        the grid (two launches; capturable)."""
        d = self._distill
        i = torch.randint(0, d.steps, (B,), device=device).long()
        return d.levels[i]

    def forward(self, img, *args, classes=None, **kwargs):
        """``classes`` (keyword, class-conditional model): the batch's labels, which go through the label drop.  Every draw
        is ``draw``'s, in the order the graph-replayed step takes them; ``p_losses`` gets every operand and draws nothing."""
        b, c, h, w = img.shape
        assert h == self.img_size and w == self.img_size, f"height and width of image must be {self.img_size}"
        noise, strength = (list(args) + [None, None])[:2]
        noise, strength = kwargs.pop("noise", noise), kwargs.pop("offset_noise_strength", strength)
        d = self.draw(img, classes, noise=noise, offset=kwargs.pop("_offset_noise", None), offset_noise_strength=strength,
                      dropout_key=kwargs.pop("_dropout_key", None), lowres_aug_t=kwargs.pop("lowres_aug_t", None),
                      lowres_noise=kwargs.pop("lowres_noise", None))
        s, eps = d.lowres or (None, None)
        return self.p_losses(img, d.t, d.noise, strength, d.classes, _offset_noise=d.offset, _dropout_key=d.dropout_key,
                             lowres_aug_t=s, lowres_noise=eps, _normalize=self.auto_normalize, _t_on_grid=True, **kwargs)

    # -- the reference's per-sample-timestep algebra (:673-705, 869-876): one lgm_extract_axpby launch each ---------
    def _axpby(self, ta, tb, td, t, x, y, sb=1.0, clip=False):
        """out = clamp?((ta[t] * x + sb * tb[t] * y) / td[t]) on dense NCHW tensors, t per sample ([B] int64)."""
        x = x.detach().float().contiguous()
        B = x.shape[0]
        assert t.shape == (B,), f"expected one timestep per sample, got {tuple(t.shape)}"
        t = t.to(device=x.device, dtype=torch.long).contiguous()
        if y is not None:
            y = y.detach().float().contiguous()
            assert y.shape == x.shape
        out = torch.empty_like(x)
        if x.numel() == 0:
            return out
        ptr = lambda a: None if a is None else a.data_ptr()  # noqa: E731
        ops.lib().lgm_extract_axpby(ptr(ta), ptr(tb), ptr(td), t.data_ptr(), x.data_ptr(), ptr(y), float(sb),
                                    1 if clip else 0, out.data_ptr(), B, x.numel() // B, self.num_timesteps,
                                    ops.stream())
        return out

    def predict_start_from_noise(self, x_t, t, noise):
        return self._axpby(self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, None, t, x_t, noise, -1.0)

    def predict_noise_from_start(self, x_t, t, x0):
        return self._axpby(self.sqrt_recip_alphas_cumprod, None, self.sqrt_recipm1_alphas_cumprod, t, x_t, x0, -1.0)

    def predict_v(self, x_start, t, noise):
        return self._axpby(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, None, t, noise, x_start, -1.0)

    def predict_start_from_v(self, x_t, t, v):
        return self._axpby(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, None, t, x_t, v, -1.0)

    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        return self._axpby(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, None, t, x_start, noise, 1.0)

    def _extract(self, a, t, ndim):
        return a.gather(-1, t).reshape(t.shape[0], *((1,) * (ndim - 1)))

    def q_posterior(self, x_start, x_t, t):
        mean = self._axpby(self.posterior_mean_coef1, self.posterior_mean_coef2, None, t, x_start, x_t, 1.0)
        return (mean, self._extract(self.posterior_variance, t, x_t.ndim),
                self._extract(self.posterior_log_variance_clipped, t, x_t.ndim))

    @torch.no_grad()
    def _guidance(self, classes, cond_scale, B, device):
        """-> (device labels or None, scale) for a sampling call; ``cond_scale=None`` is the constructor's"""
        scale = self.cond_scale if cond_scale is None else float(cond_scale)
        if scale != 1.0 and self.num_classes is None:
            raise ValueError("cond_scale != 1 needs a model built with num_classes")
        return self.model.labels(classes, B, device), scale

    def check_lowres(self, lowres, B):
        """The low-resolution image of a sampling call as the kernel reads it: float32 [B, C, img_size / r, img_size / r] on
        the device, in the data range (normalised like a training batch).  ValueError for a model without low-resolution
        conditioning, a missing image and a wrong shape."""
        if not self.lowres_cond:
            raise ValueError("lowres= was passed to a model built without lowres_cond")
        if lowres is None:
            raise ValueError("a low-resolution conditioned model samples from a low-resolution image: pass lowres=")
        n = self.img_size // self.lowres_factor
        if not torch.is_tensor(lowres) or tuple(lowres.shape) != (B, self.channels, n, n):
            got = tuple(lowres.shape) if torch.is_tensor(lowres) else type(lowres).__name__
            raise ValueError(f"lowres must be [{B}, {self.channels}, {n}, {n}] (img_size {self.img_size} / factor "
                             f"{self.lowres_factor}), got {got}")
        return lowres.to(device=self.device, dtype=torch.float32).contiguous()

    def _refuse_lowres(self, what: str):
        if self.lowres_cond:
            raise NotImplementedError(f"{what} on a low-resolution conditioned model is not built")

    def objective_tables(self):
        """the four schedule tables the objective's algebra reads, as the entry points take them (sqrt_ac .. sqrt_recipm1)"""
        return (self.sqrt_alphas_cumprod.data_ptr(), self.sqrt_one_minus_alphas_cumprod.data_ptr(),
                self.sqrt_recip_alphas_cumprod.data_ptr(), self.sqrt_recipm1_alphas_cumprod.data_ptr())

    @torch.no_grad()
    def model_predictions(self, x, t, x_self_cond=None, clip_x_start=False, rederive_pred_noise=False, classes=None,
                          cond_scale=1.0, lowres_cond_img=None, lowres_aug_t=None):
        """-> ModelPrediction(pred_noise, pred_x_start), reference :707-734.  ``rederive_pred_noise`` takes effect for
        pred_noise only (with ``clip_x_start``; otherwise pred_noise is the raw network output); for pred_x0 and pred_v the
        noise is always derived from the possibly clipped x_start.  UNet forward on the HIP engine, then ONE launch for
        both results.  ``x_self_cond`` (NCHW, ``None`` = zeros) is read by a self-conditioned network only.
        ``classes`` / ``cond_scale`` (extension): the network output is out_null + cond_scale * (out_cond - out_null), mixed
        before the objective's algebra; ``cond_scale == 1`` is one forward with the labels.
        ``dynamic_thresholding``: ``clip_x_start`` thresholds instead of clamping, in three launches - the unclipped
        predictions, ``lgm_dyn_thresh`` over the dense x_start, the predictions again with the thresholds."""
        classes, cond_scale = self._guidance(classes, cond_scale, x.shape[0], x.device)
        if cond_scale == 1.0:
            v = self.model(x, t, x_self_cond, classes, lowres_cond_img, lowres_aug_t)
        else:
            self.model._anchor(x.device)
            if self.lowres_cond and lowres_cond_img is None:
                raise ValueError("a Unet built with lowres_cond=True needs lowres_cond_img")
            v = self.model.run_nchw(x.detach().float(), t.to(x.device), False, x_self_cond, classes, cond_scale,
                                    lowres_cond_img, self.model.aug_levels(lowres_aug_t, x.shape[0], x.device))[0]
        if self.learned_variance:                    # the prediction channels; model_predictions uses no model variance
            v = v[:, :self.channels].contiguous()
        x = x.detach().float().contiguous()
        B = x.shape[0]
        t = t.to(device=x.device, dtype=torch.long).contiguous()
        pred_noise, x_start = torch.empty_like(x), torch.empty_like(x)
        tables = self.objective_tables()
        per = x.numel() // max(B, 1)
        dyn = bool(clip_x_start) and self.dynamic_thresholding and x.numel() > 0
        ops.lib().lgm_model_predictions_obj(x.data_ptr(), v.data_ptr(), t.data_ptr(), *tables, OBJECTIVES[self.objective],
                                            1 if clip_x_start and not dyn else 0, 1 if rederive_pred_noise else 0,
                                            pred_noise.data_ptr(), x_start.data_ptr(), B, per, self.num_timesteps,
                                            ops.stream())
        if dyn:
            from lgm_hip.sampler import dyn_rank
            k, w = dyn_rank(per, self.dynamic_thresholding_percentile)
            thresh = torch.empty(B, device=x.device)
            # the unclipped x_start as a one-channel pred_x0 problem: x0 = the "network output" lane, bit for bit
            ops.lib().lgm_dyn_thresh(x.data_ptr(), 1, 0, x_start.data_ptr(), 1, B, 1, per, OBJECTIVES["pred_x0"], 0.0, 0.0, 0.0,
                                     0.0, None, None, k, w, thresh.data_ptr(), ops.stream())
            ops.lib().lgm_model_predictions_thresh(x.data_ptr(), v.data_ptr(), t.data_ptr(), *tables,
                                                   OBJECTIVES[self.objective], 1 if rederive_pred_noise else 0,
                                                   pred_noise.data_ptr(), x_start.data_ptr(), B, per, self.num_timesteps,
                                                   thresh.data_ptr(), ops.stream())
        return ModelPrediction(pred_noise, x_start)

    @torch.no_grad()
    def p_mean_variance(self, x, t, x_self_cond=None, clip_denoised=True, classes=None, cond_scale=1.0, **lowres):
        x_start = self.model_predictions(x, t, x_self_cond, clip_x_start=clip_denoised, classes=classes,
                                         cond_scale=cond_scale, **lowres).pred_x_start
        mean, var, logvar = self.q_posterior(x_start=x_start, x_t=x, t=t)
        return mean, var, logvar, x_start

    # -- sampling: lgm_hip/sampler.py (one fused update kernel per step, graph replay for whole chains) -------------
    @torch.no_grad()
    def p_sample(self, x, t: int, x_self_cond=None, noise=None, classes=None, cond_scale=1.0, **lowres):
        """One ancestral step at the shared timestep ``t`` -> (pred_img, x_start), reference :748-757.  ``noise``
        (extension, for parity tests): the draw the reference takes from randn_like.  ``x_self_cond`` (NCHW, ``None`` =
        zeros): the x_start the previous step returned, for a self-conditioned network.  ``lowres`` / ``lowres_aug_t`` /
        ``lowres_noise`` (keywords, a low-resolution conditioned model): as in ``sample``."""
        from lgm_hip import sampler
        chain = sampler._Chain(self, tuple(x.shape), x, x_self_cond, classes, cond_scale, **lowres)
        if noise is None and t > 0:
            noise = torch.randn_like(x)
        sampler.p_sample_step(chain, int(t), noise)
        x0 = torch.empty(tuple(x.shape), device=chain.x.device)
        ops.nhwc_to_nchw(chain.x0, x0)
        return chain.image(False), x0

    @torch.no_grad()
    def p_sample_loop(self, shape, return_all_timesteps=False, classes=None, cond_scale=1.0, lowres=None):
        from lgm_hip import sampler
        return sampler.p_sample_loop(self, tuple(shape), return_all_timesteps, classes=classes, cond_scale=cond_scale,
                                     lowres=lowres)

    @torch.no_grad()
    def ddim_sample(self, shape, return_all_timesteps=False, classes=None, cond_scale=1.0, lowres=None):
        from lgm_hip import sampler
        return sampler.ddim_sample(self, tuple(shape), return_all_timesteps, classes=classes, cond_scale=cond_scale,
                                   lowres=lowres)

    @torch.no_grad()
    def dpm_solver_sample(self, shape, return_all_timesteps=False, classes=None, cond_scale=1.0, lowres=None):
        """DPM-Solver++ on ``dpm_time_pairs()`` (order ``dpm_order``, ``dpm_stochastic``: the SDE form), one forward per step"""
        from lgm_hip import sampler
        return sampler.dpm_solver_sample(self, tuple(shape), return_all_timesteps, classes=classes, cond_scale=cond_scale,
                                         lowres=lowres)

    @torch.no_grad()
    def sample(self, batch_size=None, return_all_timesteps=False, classes=None, cond_scale=None, lowres=None,
               lowres_aug_t=None, lowres_noise=None):
        """``classes`` (class-conditional model): one label per image, ``None`` = the null label, in one forward per step;
        ``cond_scale=None`` takes the constructor's.  ``batch_size=None``: 16, or the batch of ``lowres``.
        ``lowres`` (a low-resolution conditioned model; required there, a ValueError elsewhere): [B, C, img_size / r,
        img_size / r] in the data range.  It is normalised, upsampled and augmented at level ``lowres_aug_t`` (an int or
        one per sample; ``None`` = the constructor's ``lowres_sample_aug_t``) with one draw (``lowres_noise``, NCHW at
        ``img_size``, in its place for parity runs) into the conditioning slice, ONCE per chain."""
        kw = {}
        if self.lowres_cond or lowres is not None or lowres_aug_t is not None or lowres_noise is not None:
            if batch_size is None and torch.is_tensor(lowres):
                batch_size = lowres.shape[0]
            kw["lowres"] = dict(lowres=self.check_lowres(lowres, 16 if batch_size is None else batch_size),
                                lowres_aug_t=lowres_aug_t, lowres_noise=lowres_noise)
        batch_size = 16 if batch_size is None else batch_size
        fn = self.ddim_sample if self.is_ddim_sampling else self.p_sample_loop
        if self.sampler == "dpm++":
            fn = self.dpm_solver_sample
        scale = self.cond_scale if cond_scale is None else cond_scale
        if classes is None:
            scale = 1.0                              # out_null + s * (out_null - out_null): the null forward alone
        classes, scale = self._guidance(classes, scale, batch_size, self.device)
        return fn((batch_size, self.channels, self.img_size, self.img_size), return_all_timesteps=return_all_timesteps,
                  classes=classes, cond_scale=scale, **kw)

    @torch.no_grad()
    def inpaint(self, known, mask, jump_length=1, resamples=1, classes=None, cond_scale=None, return_all_timesteps=False):
        """Inpainting (extension; RePaint, Lugmayr et al. 2022, Algorithm 1): keep ``known`` ([B, C, H, W] in the data range,
        normalised as ``forward`` normalises) where ``mask`` ([B, 1, H, W] or [B, H, W], values in [0, 1]) is 1 and generate
        the rest.  The sampler is the one ``sample`` dispatches to; every step replaces the known region by the image noised
        to the step's level, and with ``resamples`` > 1 the chain is walked back up ``jump_length`` levels at a time
        (``lgm_hip.sampler.inpaint_walk``).  ``classes`` / ``cond_scale`` as in ``sample``."""
        from lgm_hip import sampler
        self._refuse_lowres("inpaint")
        if known.dim() != 4 or tuple(known.shape[1:]) != (self.channels, self.img_size, self.img_size):
            raise ValueError(f"known must be [B, {self.channels}, {self.img_size}, {self.img_size}], got {tuple(known.shape)}")
        b, _, h, w = known.shape
        if tuple(mask.shape) not in ((b, 1, h, w), (b, h, w)):
            raise ValueError(f"mask must be [{b}, 1, {h}, {w}] or [{b}, {h}, {w}], got {tuple(mask.shape)}")
        mask = mask.to(device=self.device, dtype=torch.float32).reshape(b, h * w)
        if mask.numel() and not bool(((mask >= 0) & (mask <= 1)).all()):
            raise ValueError("mask values must lie in [0, 1]")
        scale = self.cond_scale if cond_scale is None else cond_scale
        if classes is None:
            scale = 1.0
        classes, scale = self._guidance(classes, scale, b, self.device)
        return sampler.inpaint(self, self.normalize(known.to(self.device).float()), mask, jump_length, resamples,
                               return_all_timesteps, classes=classes, cond_scale=scale)

    @torch.no_grad()
    def vlb_terms(self, img, *, timesteps=None, noise=None, clip_denoised=True, variance="fixed_small", classes=None):
        """The variational bound of ``img`` in bits per dimension (extension; Ho et al. 2020 eq. 5, Nichol & Dhariwal 2021
        ``calc_bpd_loop``) -> ``VLBTerms(total_bpd, prior_bpd, vb, xstart_mse, mse, timesteps)``: per evaluated timestep and
        sample the term of the bound (``vb``: the KL of the two posteriors for t >= 1, the discretised-Gaussian decoder NLL at
        t = 0), mean (x0_pred - x0)^2 and mean (eps_pred - noise)^2, each [n, B]; ``prior_bpd`` [B]; ``total_bpd = vb.sum(0) +
        prior_bpd`` [B] when all T timesteps were evaluated, else None.  float64 on the host.
        ``img``: [B, C, H, W] in the data range, normalised as ``forward`` normalises.  ``timesteps``: None = T - 1 ... 0, else
        distinct ints in [0, T) in the order to evaluate.  ``noise``: one NCHW draw per evaluated timestep (parity tests).
        ``variance``: ``"fixed_small"`` (beta~_t) or ``"fixed_large"`` (beta_t), see ``lgm_hip.likelihood``; ``"learned"`` (a
        learned-variance model only): the element's own log-variance from the network's variance lanes.
        One forward per timestep, graph-replayed like sampling.  A self-conditioned network is evaluated with a zero
        self-conditioning input at every timestep: that is a Markov model of its own and therefore a valid bound (of that
        model, not of the sampler that feeds x_start forward).  A class-conditional network: ``classes=None`` is the null
        label, labels give the conditional bound; there is no guidance here - a guided output is not a probabilistic model."""
        from lgm_hip import likelihood
        self._refuse_lowres("vlb_terms")
        return likelihood.vlb_terms(self, img, timesteps=timesteps, noise=noise, clip_denoised=clip_denoised,
                                    variance=variance, classes=classes)

    @torch.no_grad()
    def nll_bpd(self, img, **kw):
        """``vlb_terms(img, **kw).total_bpd``: the bound over all T timesteps, [B] bits per dimension"""
        ts = kw.get("timesteps")
        if ts is not None and len({int(t) for t in ts}) != self.num_timesteps:
            raise ValueError("nll_bpd evaluates every timestep; use vlb_terms for a subset")
        return self.vlb_terms(img, **kw).total_bpd

    def _edit_args(self, what: str, img, classes, cond_scale, selfcond_ok: bool = False):
        """the checks every editing call makes before anything runs -> (img on the device in float32, labels, scale)"""
        self._refuse_lowres(what)
        if self.self_condition and not selfcond_ok:
            raise NotImplementedError(f"{what} on a self-conditioned model is not built: the inverse step has no x_start to "
                                      "hand on")
        want = (self.channels, self.img_size, self.img_size)
        if not torch.is_tensor(img) or img.dim() != 4 or tuple(img.shape[1:]) != want:
            got = tuple(img.shape) if torch.is_tensor(img) else type(img).__name__
            raise ValueError(f"{what} takes [B, {want[0]}, {want[1]}, {want[2]}], got {got}")
        scale = self.cond_scale if cond_scale is None else cond_scale
        if classes is None:
            scale = 1.0                              # the null forward alone, as in ``sample``
        classes, scale = self._guidance(classes, scale, img.shape[0], self.device)
        return img.to(self.device).float().contiguous(), classes, scale

    @torch.no_grad()
    def encode(self, img, steps=None, upto=None, classes=None, cond_scale=1.0, return_all_timesteps=False):
        """DDIM inversion (extension; Song et al. 2021, 4.3 and 5.4; guided-diffusion's ``ddim_reverse_sample``): the
        deterministic map from ``img`` ([B, C, S, S] in the data range, normalised as ``forward`` normalises) to the latent
        that ``decode`` turns back into it -> [B, C, S, S], the chain's state, not unnormalised.  The grid is the DDIM
        sampler's on ``steps`` steps (``None``: ``sampling_timesteps``, which must then lie below T; all T steps only by
        ``steps=T``), walked upwards (``lgm_hip.sampler.ddim_inverse_pairs``); the image is taken as the state at the grid's
        lowest level.  ``upto=k`` stops after k pairs, at level index k.  x0 is neither clipped nor thresholded on the way,
        whatever the sampler does.  ``classes`` / ``cond_scale`` as in ``sample`` (``cond_scale=None``: the constructor's): a
        guided encode is two forwards and the mix per step.  Graph-replayed like sampling."""
        from lgm_hip import sampler
        img, classes, scale = self._edit_args("encode", img, classes, cond_scale)
        return sampler.encode(self, self.normalize(img), steps, upto, return_all_timesteps, classes, scale)

    @torch.no_grad()
    def decode(self, latent, from_level=None, classes=None, cond_scale=None, steps=None, clip=True,
               return_all_timesteps=False):
        """``ddim_sample`` at eta 0 started from ``latent`` ([B, C, S, S], a state of the chain: ``encode``'s result, a slerp of
        two, noise) at level index ``from_level`` of the grid on ``steps`` steps (default: its top; ``steps`` as in ``encode``)
        -> the image in the data range.  ``clip=False`` takes x0 as predicted, as ``encode`` does: the exact way back.
        ``classes`` / ``cond_scale`` as in ``sample``."""
        from lgm_hip import sampler
        latent, classes, scale = self._edit_args("decode", latent, classes, cond_scale)
        return sampler.decode(self, latent, from_level, steps, clip, return_all_timesteps, classes, scale)

    @torch.no_grad()
    def reconstruct(self, img, steps=None, upto=None, classes=None, cond_scale=1.0):
        """``decode(encode(img))`` on one grid with the clip off both ways: what the DDIM ODE loses on ``steps`` steps"""
        z = self.encode(img, steps=steps, upto=upto, classes=classes, cond_scale=cond_scale)
        return self.decode(z, from_level=upto, classes=classes, cond_scale=cond_scale, steps=steps, clip=False)

    @torch.no_grad()
    def img2img(self, img, strength=0.5, noise=None, classes=None, cond_scale=None, return_all_timesteps=False):
        """SDEdit (extension; Meng et al. 2022): noise ``img`` ([B, C, S, S] in the data range, normalised as ``forward``
        normalises) part of the way and run the rest of the sampler ``sample`` dispatches to - the last max(1, round(strength
        N)) of its N steps, ``strength`` in (0, 1]; 1 keeps nothing of the image but its low frequencies at level T - 1.
        ``noise``: the draw of the noising ([B, C, S, S]; default: drawn).  Dynamic thresholding, guidance and learned
        variance work as they do in ``sample``; ``classes`` / ``cond_scale`` as there."""
        from lgm_hip import sampler
        img, classes, scale = self._edit_args("img2img", img, classes, cond_scale, selfcond_ok=True)
        if noise is not None:
            if tuple(noise.shape) != tuple(img.shape):
                raise ValueError(f"noise must be {tuple(img.shape)}, got {tuple(noise.shape)}")
            noise = noise.to(self.device).float().contiguous()
        return sampler.img2img(self, self.normalize(img), strength, noise, return_all_timesteps, classes=classes,
                               cond_scale=scale)

    @torch.no_grad()
    def interpolate(self, x1, x2, t=None, lam=0.5, classes=None, cond_scale=1.0, method="stochastic", steps=None,
                    upto=None):
        """reference :847-867: noise both images to step t, blend, walk the ancestral chain back to 0 (no unnormalise).
        ``method="ddim"`` (extension; Song et al. 2021, fig. 6): ``encode`` both images (given as the reference's form takes
        them: already normalised), slerp the latents with ``lam`` (a float or a [B] tensor) on the device, ``decode`` with the
        clip off - deterministic, and the blend keeps the latents' norm, which a lerp at ``lam = 0.5`` does not.  ``t`` is
        not read there; ``steps`` and ``upto`` as in ``encode`` (``upto``: blend at that level of the grid, not at its top)."""
        from lgm_hip import sampler
        if method not in ("stochastic", "ddim"):
            raise ValueError(f"method must be 'stochastic' or 'ddim', got {method!r}")
        if method == "ddim":
            x1, classes_d, scale = self._edit_args("interpolate(method='ddim')", x1, classes, cond_scale)
            x2 = self._edit_args("interpolate(method='ddim')", x2, classes, cond_scale)[0]
            return sampler.interpolate_ddim(self, x1, x2, lam, steps, classes_d, scale, upto)
        self._refuse_lowres("interpolate")
        b = x1.shape[0]
        t = self.num_timesteps - 1 if t is None else int(t)
        assert x1.shape == x2.shape
        tb = torch.full((b,), t, device=x1.device, dtype=torch.long)
        xt1, xt2 = self.q_sample(x1, tb), self.q_sample(x2, tb)
        img = (1 - lam) * xt1 + lam * xt2
        return sampler.p_sample_loop(self, tuple(img.shape), init_noise=img, start=t, unnormalize=False, classes=classes,
                                     cond_scale=cond_scale)


def hip_loss_forward(gd: "GaussianDiffusion", img, t, noise, normalize: bool, save: bool, offset=None,
                     strength: float = 0.0, self_cond=False, classes=None, dropout_key=None, lowres=None):
    """q_sample + UNet + the objective's target + weighted MSE on the HIP engine.  Returns (loss[1], ctx).
    ``offset`` ([B, C] or None) / ``strength``: offset noise, added to ``noise`` inside the q_sample kernel.
    ``self_cond`` (self-conditioned network only): ``True`` = estimate pass first (``hip_loss_estimate``), a tensor = that
    NCHW estimate.  ``classes``: device labels (``Unet.labels``) both passes of a class-conditional network read.
    ``dropout_key``: the step's key (``GaussianDiffusion.draw_dropout_key``) both passes read, None = neither drops.
    ``lowres``: (s, eps_aug) of a low-resolution conditioned network (``GaussianDiffusion.draw_lowres``)."""
    q = gd.qsample(img, StepDraws(t, noise, offset, classes, dropout_key, lowres), normalize, strength)
    if gd.model.self_condition:
        if torch.is_tensor(self_cond):
            assert self_cond.shape == img.shape
            ops.nchw_to_nhwc(self_cond.detach().float().contiguous(), gd.model.sc_slice(q.xt))
        elif self_cond:
            hip_loss_estimate(gd, q.xt, q.t, classes, dropout_key)
    return hip_loss_network(gd, q.xt, q.target, q.img, q.t, q.noise, q.offset, save, classes, normalize, dropout_key,
                            q.lowres_s)


def hip_loss_distill(gd: "GaussianDiffusion", q: QSample, classes=None):
    """The distillation target over ``q.target`` (``GaussianDiffusion.distill_from``): the teacher's forward at (z_t, t) on the
    student's own input buffer - both networks read the same layout -, ``lgm_distill_half_step`` into the teacher's second input
    buffer, its forward at (z_t', t'), ``lgm_distill_target``.  No activation is saved, nothing is drawn; ``classes``: the device
    labels the student's pass reads.  The teacher's derived weight copies are refreshed by the first call after its weights
    were set, not per step: they are frozen."""
    d, net = gd._distill, gd.model
    tnet = d.teacher
    B, H, W, _ = q.xt.shape
    tnet.prepare_hip(q.xt.device)
    assert (tnet.in_pitch, tnet.x_off) == (net.in_pitch, net.x_off), "teacher and student read one input layout"
    to, so = OBJECTIVES[d.objective], OBJECTIVES[gd.objective]
    out1, _ = tnet.forward_nhwc(q.xt, q.t, False, d.stale, classes)
    d.stale = False
    xmid = tnet.input_buffer(B, H, W, q.xt)
    t_mid = torch.empty_like(q.t)
    ops.distill_half_step(q.xt, net.x_off, out1, q.t, d.table, to, d.clip, xmid, tnet.x_off, t_mid, net.channels)
    out2, _ = tnet.forward_nhwc(xmid, t_mid, False, False, classes)
    ops.distill_target(q.xt, net.x_off, xmid, tnet.x_off, out2, q.t, d.table, to, so, d.clip, q.target, net.channels)
    return q


def hip_loss_estimate(gd: "GaussianDiffusion", xt, t, classes=None, dropout_key=None):
    """The estimate pass of a self-conditioned training step (:901-905): the network without saved activations on the input
    buffer whose self-conditioning slice is zero, then ONE launch that writes the unclipped x_start into that slice.
    ``dropout_key``: the step's key; this is pass 1 of the dropout mask."""
    net = gd.model
    B, H, W, _ = xt.shape
    out, _ = net.forward_nhwc(xt, t, False, True, classes, dropout_key, 1)
    ops.lib().lgm_selfcond_estimate(xt.data_ptr(), net.in_pitch, net.x_off, net.sc_off, out.data_ptr(), ops.pitch(out),
                                    t.data_ptr(), *gd.objective_tables(), OBJECTIVES[gd.objective], B, net.channels, H * W,
                                    gd.num_timesteps, ops.stream())


def hip_loss_qsample(gd: "GaussianDiffusion", img, t, noise, normalize: bool, offset=None, strength: float = 0.0,
                     lowres=None):
    """x_t into the network's input buffer and the objective's target: one launch.  A self-conditioned network's buffer gets
    x_t in its x slice and zeros in its self-conditioning slice; any other network's buffer is the x slice alone
    (``in_pitch = r4(C)``, ``x_off = 0``, ``sc_off = -1``).  A low-resolution conditioned network (``lowres`` = (s, eps_aug)): a
    second launch writes the conditioning slice from the same ``img`` - area average, bilinear upsample, normalisation and
    augmentation in one pass, the low-resolution tensor never reaches memory (lgm_lowres_cond)."""
    net = gd.model
    B, C, H, W = img.shape
    Cp = _r4(C)
    img = img.detach().float().contiguous()
    noise = noise.detach().float().contiguous()
    t = t.contiguous()
    xt = net.input_buffer(B, H, W, img)
    target = ops.new((B, H, W, Cp), img)
    if offset is not None:
        offset = offset.detach().float().contiguous()
        assert offset.shape == (B, C), f"offset noise is one value per (sample, channel), got {tuple(offset.shape)}"
    ops.lib().lgm_qsample_target_slice(img.data_ptr(), noise.data_ptr(), None if offset is None else offset.data_ptr(),
                                       float(strength), t.data_ptr(), gd.sqrt_alphas_cumprod.data_ptr(),
                                       gd.sqrt_one_minus_alphas_cumprod.data_ptr(), 1 if normalize else 0,
                                       OBJECTIVES[gd.objective], xt.data_ptr(), net.in_pitch, net.x_off, net.sc_off,
                                       target.data_ptr(), Cp, B, C, H * W, Cp, ops.stream())
    if not net.lowres_cond:
        return QSample(xt, target, img, noise, t, offset)
    s, eps = lowres
    s, eps = s.contiguous(), eps.detach().float().contiguous()
    ops.lowres_cond(xt, net.cond_off, C, gd.lowres_factor, img=img, eps=eps, s=s, sqrt_ac=gd.sqrt_alphas_cumprod,
                    sqrt_1mac=gd.sqrt_one_minus_alphas_cumprod, normalize=normalize)
    # (eps is read by this launch alone: nothing behind it keeps it)
    return QSample(xt, target, img, noise, t, offset, s)


class LossContext:
    """What the loss forward hands to its backward, for all four loss forms.  ``xt`` / ``normalize`` / ``per`` (the per-sample
    terms [2, B] = (loss_weight mse_b, vb_b)) belong to the hybrid loss of a learned-variance network and stay None for the
    weighted MSE; ``wb`` ([B], the weights iw[t_b]) is there when the forward ran under a loss-aware timestep sampler.
    ``shape``: (B, C, H, W) of ``img``; ``tape``: None when the forward saved no activations."""
    __slots__ = ("gd", "tape", "out", "target", "t", "shape", "img", "noise", "offset", "xt", "normalize", "per", "wb")

    def __init__(self, gd, tape, out, target, t, shape, img, noise, offset):
        self.gd, self.tape, self.out, self.target, self.t, self.shape = gd, tape, out, target, t, shape
        self.img, self.noise, self.offset = img, noise, offset
        self.xt = self.normalize = self.per = self.wb = None


def _loss_form(c: LossContext):
    """-> ((forward, backward) entry point of ``c``'s loss form - the *_iw pair when the forward leaves weights in ``c.wb`` -,
    the operands the two share in their order (up to ``vb_weight`` / ``loss_weight``), their (B, C, HW[, Cpad]))"""
    L, gd, (B, C, H, W), weighted = ops.lib(), c.gd, c.shape, c.wb is not None
    if gd.learned_variance:
        fns = (L.lgm_hybrid_loss_fwd_iw, L.lgm_hybrid_loss_bwd_iw) if weighted else (L.lgm_hybrid_loss_fwd, L.lgm_hybrid_loss_bwd)
        return fns, (c.out.data_ptr(), ops.pitch(c.out), c.target.data_ptr(), ops.pitch(c.target), c.img.data_ptr(),
                     1 if c.normalize else 0, c.xt.data_ptr(), gd.model.in_pitch, gd.model.x_off, c.t.data_ptr(),
                     *gd.objective_tables(), gd.loss_weight.data_ptr(), gd.learned_table.data_ptr(), gd.num_timesteps,
                     OBJECTIVES[gd.objective], float(gd.vb_loss_weight)), (B, C, H * W)
    fns = (L.lgm_weighted_mse_fwd_iw, L.lgm_weighted_mse_bwd_iw) if weighted else (L.lgm_weighted_mse_fwd, L.lgm_weighted_mse_bwd)
    return fns, (c.out.data_ptr(), c.target.data_ptr(), _r4(C), c.t.data_ptr(), gd.loss_weight.data_ptr()), (B, C, H * W, _r4(C))


def hip_loss_network(gd: "GaussianDiffusion", xt, target, img, t, noise, offset, save: bool, classes=None, normalize=None,
                     dropout_key=None, lowres_s=None, net_t=None):
    """The pass the gradient is taken through + weighted MSE.  Returns (loss[1], ctx).  A learned-variance network: the hybrid
    loss instead (lgm_hybrid_loss_fwd: the same MSE over the prediction lanes + vb_loss_weight times the bound's term), ``ctx``
    (``LossContext``) then also holds the per-sample terms, x_t and ``normalize`` - whether ``img`` is still in the data range
    (``None``: the diffusion's auto_normalize, what the graph-replayed step hands its q_sample).  ``dropout_key``: the step's key;
    this is pass 0 of the dropout mask.  ``net_t``: the time the network reads where it is not ``t`` (``QSample.net_t``)."""
    B, C, H, W = img.shape
    hybrid = gd.learned_variance
    out, tape = gd.model.forward_nhwc(xt, t if net_t is None else net_t, save, True, classes, dropout_key, 0, lowres_s)
    loss = ops.new((1,), img)
    ctx = LossContext(gd, tape, out, target, t, (B, C, H, W), img, noise, offset)
    # a loss-aware timestep sampler (training mode): the *_iw forms weight sample b by iw[t_b] and leave that weight in ``wb``
    # for the backward, then ONE launch records the unweighted per-sample losses and rebuilds the plan of the next draw
    ts = gd.active_t_sampler()
    ts = ts if ts is not None and ts.loss_aware else None
    if ts is not None:
        ts.ensure_plan()
        ctx.wb = ops.new((B,), img)
    per = ops.new((2, B) if hybrid else (B,), img)
    if hybrid:                                       # (the weighted MSE's backward reads no per-sample term: not kept)
        ctx.xt, ctx.normalize, ctx.per = xt, bool(gd.auto_normalize if normalize is None else normalize), per
    (fwd, _), head, dims = _loss_form(ctx)
    if ts is None:
        fwd(*head, *dims, per.data_ptr(), loss.data_ptr(), ops.stream())
    else:                                            # (the hybrid operands already hold the tables' length)
        table = (ts.iw.data_ptr(),) if hybrid else (ts.iw.data_ptr(), gd.num_timesteps)
        fwd(*head, *table, *dims, per.data_ptr(), ctx.wb.data_ptr(), loss.data_ptr(), ops.stream())
        ts.record(t, per, 2 if hybrid else 1, gd.vb_loss_weight if hybrid else 0.0)
    return loss, ctx


def hip_loss_backward_begin(ctx: LossContext, gl):
    """Loss gradient (``gl``: device scalar [1] = dL/dloss) and the opened UNet backward (``Unet.backward_run``)."""
    if ctx.tape is None:
        raise RuntimeError("p_losses forward ran without saving activations")
    gout = ops.new(ctx.out.shape, ctx.out)
    (_, bwd), head, dims = _loss_form(ctx)
    weights = () if ctx.wb is None else (ctx.wb.data_ptr(),)     # what the forward left under a loss-aware timestep sampler
    bwd(*head, *weights, gl.data_ptr(), *dims, gout.data_ptr(), ops.stream())
    st = ctx.gd.model.backward_begin(ctx.tape, gout)
    # what the launch read: let go of with the phase that reads ``gout``, also when ``ctx`` is gone by then
    st.held += [ctx.out, ctx.target] + ([ctx.img, ctx.xt] if ctx.gd.learned_variance else []) + [ctx.wb]
    return st


class _LossFn(torch.autograd.Function):
    """A diffusion's training loss - ``loss_forward(save) -> (loss[1], LossContext)``: ``hip_loss_forward``, or
    ``edm.edm_loss_forward`` - with the hand-written backward."""

    @staticmethod
    def forward(ctx, anchor, loss_forward):
        loss, ctx.stuff = loss_forward(bool(ctx.needs_input_grad[0]))
        return loss.view(())

    @staticmethod
    def backward(ctx, gloss):
        gl = gloss.detach().float().reshape(1).contiguous()
        ctx.stuff.gd.model.backward_run(hip_loss_backward_begin(ctx.stuff, gl))
        ctx.stuff = None
        return None, None


# ----------------------------------------------------------------------------------------
# LightningModule  (reference :949-1094)
# ----------------------------------------------------------------------------------------
class DiffusionModule(LightningModule):
    """What ``DDPM`` and ``EDM`` (edm.py) share: the EMA around the diffusion (keys ``ema.online_model.*`` /
    ``ema.ema_model.*``), the training and validation loss, logging, periodic sampling, the optimizer and the graph-replayed
    step.  A subclass's ``__init__`` calls ``save_hyperparameters()`` (it reads the caller's arguments) and ``_wrap``."""

    def _wrap(self, diffusion, img_channels, img_size, ema_decay, ema_update_every):
        self.channels, self.img_size = img_channels, img_size
        self.ema = EMA(diffusion, beta=ema_decay, update_every=ema_update_every)
        self.ema.ema_model.model.dropout = 0.0       # the shadow is what samples and validates: it never drops
        self.sample_every = 1000          # reference: every 1000 steps on rank 0 (:1025)
        self.last_samples = None

    def prepare_hip(self, device):
        self.ema.online_model.model.prepare_hip(device)
        self.ema.ema_model.model.prepare_hip(device)
        if self.ema.online_model._distill is not None:
            self.ema.online_model._distill.teacher.prepare_hip(device)

    def ddp_buffers(self):
        """Buffers training writes (re-broadcast from rank 0 before every forward, lgm_hip.lightning.BufferSync): none —
        the 13 schedule tables are constants and the EMA shadow is updated identically on every rank."""
        return []

    def _shadow(self):
        """the diffusion ``_log_sample`` samples from - the EMA weights -, in evaluation mode"""
        self.ema.ema_model.eval()
        return self.ema.ema_model

    def _batch_loss(self, model, data, y):
        return model(data, classes=y) if self.num_classes is not None else model(data)

    def _common_step(self, batch, mode: str):
        assert mode in ["train", "val", "test"], f"Invalid mode: {mode}"
        data, y = batch
        loss = self._batch_loss(self.ema.model if self.training else self.ema.ema_model, data, y)
        self.log(f"{mode}_loss", loss, prog_bar=True, logger=True, sync_dist=multi_rank())
        if self.sample_every and self.global_step % self.sample_every == 0 and _is_master():
            self._log_sample()
        return loss

    def _log_images(self):
        """``last_samples`` to the logger, where there is one that takes images"""
        logger = getattr(self, "logger", None)
        if logger is not None and hasattr(logger, "experiment"):
            try:  # W&B is optional
                import wandb  # type: ignore
                logger.experiment.log({"Random Generation": [wandb.Image(self.last_samples)]}, step=self.global_step)
            except Exception:  # noqa
                pass

    def training_step(self, batch):
        return self._common_step(batch, "train")

    def on_train_batch_end(self, outputs, batch, batch_idx):
        self.ema.update()

    def validation_step(self, batch):
        return self._common_step(batch, "val")

    def configure_optimizers(self):
        return FusedAdam(self.ema.model.parameters(), lr=self.hparams.lr, betas=self.hparams.betas)

    def make_fast_step(self, opt, world: int = 1, use_graph: bool = True, accumulate: int = 1):
        """The step object ``MiniTrainer.fit`` drives instead of training_step/backward/step: overlapped
        bucketed gradient exchange + HIP-graph replay (what bench.py times), eager fallback inside."""
        from lgm_hip.graph import DDPMFastStep
        return DDPMFastStep(self, opt, world, use_graph, accumulate=accumulate)


class DDPM(DiffusionModule):
    def __init__(self, img_channels: int = 3, img_size: int = 64, dim: int = 64, diffusion_timesteps: int = 1000,
                 sampling_timesteps: Optional[int] = None, lr: float = 2e-5, betas: Tuple[float, float] = (0.9, 0.99),
                 ema_update_every: int = 10, ema_decay: float = 0.995, objective: str = "pred_v",
                 beta_schedule: str = "sigmoid", offset_noise_strength: float = 0.0, min_snr_loss_weight: bool = False,
                 min_snr_gamma: float = 5, self_condition: bool = False, dropout: float = 0.0,
                 lowres_cond: bool = False, lowres_factor: int = 4, lowres_aug_levels: Optional[int] = None,
                 lowres_sample_aug_t: Optional[int] = None, distill_steps: Optional[int] = None,
                 num_classes: Optional[int] = None,
                 cond_drop_prob: float = 0.1, t_sampler: str = "uniform", t_sampler_history: int = 10,
                 t_sampler_uniform_prob: float = 0.001, dynamic_thresholding: bool = False,
                 dynamic_thresholding_percentile: float = 0.995, learned_variance: bool = False,
                 vb_loss_weight: float = 0.001, cond_scale: float = 1.0, sampler: str = "auto",
                 dpm_order: int = 2, dpm_stochastic: bool = False):
        """``num_classes`` (extension): class-conditional training on the batches' labels with classifier-free guidance;
        ``cond_drop_prob`` / ``cond_scale`` are read with it only.  ``sampler`` / ``dpm_order`` / ``dpm_stochastic``
        (extension): ``"dpm++"`` samples with DPM-Solver++ in ``sampling_timesteps`` steps (GaussianDiffusion).
        ``dynamic_thresholding`` / ``dynamic_thresholding_percentile`` (extension): the samplers threshold x0 per sample
        instead of clamping it to [-1, 1] (GaussianDiffusion).  ``learned_variance`` / ``vb_loss_weight`` (extension): the
        network gets the variance head and trains on the hybrid loss (GaussianDiffusion); ``vb_loss_weight`` is read with it
        only.  ``t_sampler`` / ``t_sampler_history`` / ``t_sampler_uniform_prob`` (extension): how training draws its
        timesteps, ``"uniform"``, ``"stratified"`` or ``"loss_second_moment"`` (GaussianDiffusion); the sampler's state belongs
        to the model that trains - the EMA shadow has none, each rank keeps its own - and is saved under
        ``ema.online_model.t_sampler.history`` / ``.counts``.  New keywords stand in front of those that tests pin (the tail
        from ``dynamic_thresholding`` on: tests/test_dpmpp_host.py, tests/test_learned_sigma_host.py); pass everything from
        ``num_classes`` on by keyword.  ``dropout`` (extension; Ho et al. 2020 use 0.1 on CIFAR-10): the probability with
        which the ResnetBlocks drop in the network passes of the training loss (``Unet``); the EMA shadow never drops.
        ``lowres_cond`` / ``lowres_factor`` / ``lowres_aug_levels`` / ``lowres_sample_aug_t`` (extension): a super-resolution
        stage of a cascade - the model trains on batches at ``img_size`` and conditions on their own ``lowres_factor`` times
        smaller, noise-augmented version (``Unet`` / ``GaussianDiffusion``); ``upsample`` super-resolves a given image and
        ``sample_cascade`` runs a base model and its stages end to end.
        ``distill_steps`` (extension; progressive distillation, Salimans & Ho 2022): ``None`` = a plain model; N = the module
        starts as the student of a round at N sampling steps whose teacher is a frozen copy of its own weights
        (``start_distillation(N)``) - load the teacher's checkpoint into it, or pass ``--distill_from`` to train.py."""
        super().__init__()
        self.save_hyperparameters()
        self.num_classes = num_classes
        model = Unet(dim=dim, channels=img_channels, self_condition=self_condition, num_classes=num_classes,
                     dropout=dropout, **(dict(learned_variance=True) if learned_variance else {}),
                     **(dict(lowres_cond=True) if lowres_cond else {}))
        cond = dict(cond_drop_prob=cond_drop_prob, cond_scale=cond_scale) if num_classes is not None else {}
        if learned_variance:
            cond["vb_loss_weight"] = vb_loss_weight
        cond.update(t_sampler=t_sampler, t_sampler_history=t_sampler_history, t_sampler_uniform_prob=t_sampler_uniform_prob)
        if lowres_cond:
            cond.update(lowres_factor=lowres_factor, lowres_aug_levels=lowres_aug_levels, lowres_sample_aug_t=lowres_sample_aug_t)
        diffusion_model = GaussianDiffusion(model, img_size=img_size, timesteps=diffusion_timesteps,
                                            sampling_timesteps=sampling_timesteps, objective=objective,
                                            beta_schedule=beta_schedule, offset_noise_strength=offset_noise_strength,
                                            min_snr_loss_weight=min_snr_loss_weight, min_snr_gamma=min_snr_gamma,
                                            sampler=sampler, dpm_order=dpm_order, dpm_stochastic=dpm_stochastic,
                                            dynamic_thresholding=dynamic_thresholding,
                                            dynamic_thresholding_percentile=dynamic_thresholding_percentile, **cond)
        self.lowres_cond, self.lowres_factor = bool(lowres_cond), int(lowres_factor)
        self._cond_images = None          # a low-resolution conditioned model: the last batch seen, for _log_sample
        self._wrap(diffusion_model, img_channels, img_size, ema_decay, ema_update_every)
        self.bpd_every = 0                # > 0: validation_step also logs val_bpd on every bpd_every-th batch (extension)
        self._val_batches = 0
        if distill_steps is not None:
            self.start_distillation(distill_steps)

    # -- progressive distillation (extension; GaussianDiffusion.distill_from) ---------------------------------------
    @torch.no_grad()
    def start_distillation(self, steps: int, teacher=None, source: str = "ema"):
        """Begin a round: this module becomes the student at ``steps`` sampling steps of a frozen copy of ``teacher`` - another
        ``DDPM``, or ``None`` = this module's own weights - taken from its EMA shadow (``source="ema"``) or its online weights
        (``"online"``).  As in the paper the student starts from the teacher: the online weights AND the EMA shadow are set to
        the teacher's, the EMA clock starts again and the optimizer moments are dropped.  The refusals are
        ``GaussianDiffusion.distill_from``'s.  A step object made before (``make_fast_step``) captures its graphs anew."""
        if source not in ("ema", "online"):
            raise ValueError(f"source must be 'ema' or 'online', got {source!r}")
        src = self if teacher is None else teacher
        tgd = src.ema.ema_model if source == "ema" else src.ema.online_model
        online, shadow = self.ema.online_model, self.ema.ema_model
        online.distill_from(tgd, steps)              # (the copy is made here: ``tgd`` may be one of the two set below)
        weights = online._distill.teacher.state_dict()
        for gd in (online, shadow):
            gd.model.load_state_dict(weights)
        shadow.set_sampling_steps(steps)
        self.ema.step.zero_()
        self.ema.initted.fill_(False)
        self.ema._step_py, self.ema._initted_py = 0, False
        for o in getattr(self, "_optimizers", None) or []:
            getattr(o, "_opt", o)._flat_state.clear()            # FusedAdam: the moments and the step count of every flat buffer
        self.hparams["distill_steps"] = int(steps)
        return self

    def halve(self, source: str = "online"):
        """The next round: the current student (its online weights, or ``source="ema"``) becomes the teacher of a student at
        ``distill_steps // 2``.  ValueError without a teacher attached, at one step, and at an odd step count (the student's grid
        is then not the one a teacher of ``2 * (steps // 2)`` steps walks)."""
        n = self.ema.online_model.distill_steps
        if n is None:
            raise ValueError("halve() needs a distillation round: call start_distillation first")
        if n == 1 or n % 2:
            raise ValueError(f"a student of {n} step{'s' if n > 1 else ''} cannot be halved")
        return self.start_distillation(n // 2, None, source)

    def _common_step(self, batch, mode: str):
        if self.lowres_cond:
            self._cond_images = batch[0]  # what _log_sample super-resolves: the batch at hand, downsampled
        return super()._common_step(batch, mode)

    def _batch_loss(self, model, data, y):
        # a distillation round validates the shadow against the round's teacher: the shadow itself carries none, it borrows the
        # online model's for the call
        borrow = model._distill is None and self.ema.online_model._distill is not None
        if borrow:
            model._distill = self.ema.online_model._distill
        try:
            return super()._batch_loss(model, data, y)
        finally:
            if borrow:
                model._distill = None

    @torch.no_grad()
    def _log_sample(self):
        shadow = self._shadow()
        if self.lowres_cond:
            # a super-resolution stage has nothing to sample from without an image: it super-resolves the downsampled
            # batch of the step that logs (validation_step: the validation batch)
            if self._cond_images is None:
                return
            data = self._cond_images[:64].to(shadow.device).float()
            low = torch.nn.functional.avg_pool2d(data, self.lowres_factor)
            kw = {}
            if self.num_classes is not None:
                kw["classes"] = torch.arange(low.shape[0], device=low.device) % self.num_classes
            self.last_samples = shadow.sample(lowres=low, **kw)
        elif self.num_classes is not None:             # every class in turn, at the configured guidance scale
            classes = torch.arange(64, device=shadow.device) % self.num_classes
            self.last_samples = shadow.sample(batch_size=64, classes=classes)
        else:
            self.last_samples = shadow.sample(batch_size=64)
        self._log_images()

    @torch.no_grad()
    def inpaint(self, known, mask, **kw):
        """``GaussianDiffusion.inpaint`` of the diffusion ``_log_sample`` samples from (the EMA weights)"""
        return self._shadow().inpaint(known, mask, **kw)

    @torch.no_grad()
    def encode(self, img, **kw):
        """``GaussianDiffusion.encode`` of the diffusion ``_log_sample`` samples from (the EMA weights)"""
        return self._shadow().encode(img, **kw)

    @torch.no_grad()
    def decode(self, latent, **kw):
        """``GaussianDiffusion.decode`` of the diffusion ``_log_sample`` samples from (the EMA weights)"""
        return self._shadow().decode(latent, **kw)

    @torch.no_grad()
    def reconstruct(self, img, **kw):
        """``GaussianDiffusion.reconstruct`` of the diffusion ``_log_sample`` samples from (the EMA weights)"""
        return self._shadow().reconstruct(img, **kw)

    @torch.no_grad()
    def img2img(self, img, **kw):
        """``GaussianDiffusion.img2img`` of the diffusion ``_log_sample`` samples from (the EMA weights)"""
        return self._shadow().img2img(img, **kw)

    @torch.no_grad()
    def upsample(self, img_low, **kw):
        """``GaussianDiffusion.sample(lowres=img_low, **kw)`` of the diffusion ``_log_sample`` samples from (the EMA weights):
        ``img_low`` [B, C, img_size / lowres_factor, img_size / lowres_factor] in the data range -> [B, C, img_size, img_size]"""
        return self._shadow().sample(lowres=img_low, **kw)

    @torch.no_grad()
    def bits_per_dim(self, img, classes=None, **kw):
        """``GaussianDiffusion.nll_bpd`` of the diffusion ``_log_sample`` samples from (the EMA weights): [B] bits per dimension"""
        shadow = self._shadow()
        if shadow.learned_variance:                  # the variance the model was trained to predict, unless the caller says
            kw.setdefault("variance", "learned")
        return shadow.nll_bpd(img, classes=classes, **kw)

    def validation_step(self, batch):
        loss = super().validation_step(batch)
        if self.bpd_every > 0:
            if self._val_batches % self.bpd_every == 0:
                data, y = batch
                bpd = self.bits_per_dim(data, classes=y if self.num_classes is not None else None)
                self.log("val_bpd", bpd.mean().float(), prog_bar=True, logger=True, sync_dist=multi_rank())
            self._val_batches += 1
        return loss


@torch.no_grad()
def sample_cascade(stages, batch_size, classes=None):
    """A cascade end to end in the data range: ``stages[0]`` (a ``DDPM`` without low-resolution conditioning) samples
    ``batch_size`` images, every later stage (``DDPM(lowres_cond=True)`` whose ``img_size / lowres_factor`` is the size of the
    stage below) super-resolves what the stage below returned (``DDPM.upsample``).  ``classes``: the labels every
    class-conditional stage samples with.  Everything stays on the device; each stage samples under its EMA weights."""
    if not stages:
        raise ValueError("sample_cascade needs at least a base model")
    base = stages[0]
    if getattr(base, "lowres_cond", False):
        raise ValueError("the first stage of a cascade is a base model: it has no low-resolution conditioning")
    size = base.img_size
    for k, st in enumerate(stages[1:], 1):
        if not getattr(st, "lowres_cond", False):
            raise ValueError(f"stage {k} of the cascade is not a low-resolution conditioned model")
        if st.img_size != size * st.lowres_factor or st.channels != base.channels:
            raise ValueError(f"stage {k} upsamples {st.img_size // st.lowres_factor} x {st.img_size // st.lowres_factor} "
                             f"images of {st.channels} channels, the stage below returns {size} x {size} of {base.channels}")
        size = st.img_size
    label = lambda m: dict(classes=classes) if m.num_classes is not None and classes is not None else {}  # noqa: E731
    base.ema.ema_model.eval()
    img = base.ema.ema_model.sample(batch_size=batch_size, **label(base))
    for st in stages[1:]:
        img = st.upsample(img, **label(st))
    return img


def _is_master() -> bool:
    import torch.distributed as dist
    return (not dist.is_available()) or (not dist.is_initialized()) or dist.get_rank() == 0
