"""The ledger of the Winograd kernels: every name the library can note from winograd.hip, winograd4.hip, winograd4l.hip and
winograd4_wgrad.hip is RUN at the smallest shape that reaches it through the C entry points that bypass the `preferred`
tables, `lgm_last_kernel()` is compared for EQUALITY (full strings, template arguments included), and every output element
is bounded against float64 in units of 2^-24 * S_W (oracle/winograd.py: the same algorithm on absolute values; tolerance
measured on the float32 CPU Winograd by tests/test_cpu_wino_bounds.py, four times that for the kernels).

Every activation operand (x, gy, the residual) is a channel slice of a wider allocation whose other floats are all NaN: the
channels beside the slice, a full image row before the first pixel and one after the last.  The kernels get their zero
padding from buffer bounds and masks; a read of row -1, row H, the neighbouring image or the neighbouring channels that is
then multiplied by 0 shows as a NaN in the output.  Outputs are slices of NaN-filled buffers too (guards must stay NaN), and
a second launch must give the same bits.

Rows whose unit packs several images - the backward pair launch included - run a second time with all images zero but one
(no bias, no residual): the zero images' outputs must be exactly 0, whatever the tolerance.

Weight gradients go through lgm_conv_wgrad / lgm_conv_wgrad_deferred / lgm_conv3x3_wino_wgradn / lgm_conv3x3_wino4_wgrad with a
NaN-filled slab workspace of their own per launch: a slab, or an element of one, that a launch does not write is a NaN in
the reduced gradient.  Every layer of a grouped launch has its own inputs (and every second one another geometry of the same
map class), so a layer that is handed another layer's operands or output fails its score.

Rows that need an environment switch the library reads once per process run in a fresh child per switch, one at a time; a
child that ends by signal, abort or timeout fails the test and no further child starts in the session.

The completeness tests need no GPU: every registry name of the four files is a key of LEDGER, and no key is a name the
library never notes.  The debug / attribution builds (lgm_wino*_set_debug_buffer) note the plain name and are documented
to give wrong results: out of scope."""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":          # child process of test_switch_rows: the package is not on the path yet
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "lightning-generative-models_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from oracle import bounds
from oracle import winograd as OW

PREFIXES = ("lgmwino::", "lgmwino4::", "lgmwino4l::", "lgmwino4w::")
NAN = float("nan")


def R(name, entry, geom, why, env=None, **opts):
    opts.setdefault("family", "plain")
    return {"name": name, "entry": entry, "geom": tuple(geom), "why": why, "env": env, "opts": opts}


def _c2(G):
    return f"lgmwino::wino_conv_kernel<{G}, false, 0>"


def _c4(cls):
    return f"lgmwino4::wino4_conv_kernel<{cls}, false, 0, false>"


def _l4(cls):
    return f"lgmwino4l::wino4l_conv_kernel<{cls}, false>"


# geometry = (B, H, W, Cin, Cout).  opts: family; yx (input gradient: gathers Cout, produces Cin); bias / res; split = the
# reduction is expected split (True) / unsplit (False) - checked against the library's own workspace / plane answers;
# planned = the split count the workspace is sized for; multi = the unit packs several images; light = lgm_wino4_set_light mode of
# the row (default 0: 32-tile workgroups).
LEDGER = []
# ---- F(2x2) forward / input gradient (winograd.hip): plan_unit gives 64 tiles = 2x2 tiles of 16 images (4x4 maps), 4x4 tiles
#      of 4 images (8x8), 8x8 tiles of one image (>= 16x16).  lgm_wino_splits: at least two phases (16 channels) per split.
for _G, (_B, _H) in {2: (16, 4), 4: (4, 8), 8: (1, 16)}.items():
    _m = _G < 8
    LEDGER += [
        R(_c2(_G), "wino", (_B, _H, _H, 8, 64), "gathers 8 channels, the least lgm_wino_supported takes: one phase, unsplit "
          "(U built on the host: lgm_wino_weights works in 32 x 32 blocks)", bias=True, split=False, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 8), "input gradient gathering Cout = 8", yx=True, res=True, split=False, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 64), "C = 64: 8 phases split, through the reducer", family="offset", bias=True,
          res=True, split=True, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 64), "input gradient, split, through the reducer", family="offset", yx=True,
          bias=True, res=True, split=True, multi=_m),
        R(_c2(_G), "wino_partial", (_B, _H, _H, 64, 64), "the planes stay in the workspace; summed here in the reducer's order",
          bias=True, split=True, multi=_m),
        R(_c2(_G), "wino_partial", (_B, _H, _H, 64, 64), "input-gradient planes", yx=True, split=True, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 88, 64), "11 phases: four splits of 3, 3, 3 and 2 phases, the last ragged (five splits of "
          "three phases would leave the fifth empty, so lgm_wino_splits skips that count)", bias=True, split=True, planned=4, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 88), "input gradient over 11 phases: ragged last split", yx=True, res=True, split=True,
          planned=4, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 64), "tile-edge impulses, one tap", family="impulse", bias=True, split=True, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 64), "tile-edge impulses through the mirrored taps", family="impulse", yx=True,
          split=True, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 64, 128), "two channel blocks", bias=True, res=True, split=True, multi=_m),
        R(_c2(_G), "wino", (_B, _H, _H, 128, 64), "input gradient, two channel blocks", yx=True, split=True, multi=_m),
    ]
LEDGER += [
    R(_c2(2), "wino", (32, 4, 4, 64, 64), "two image groups: tile_fastest on (whole-image units, nbg = 2)", bias=True, res=True,
      split=True, multi=True),
    R(_c2(2), "wino", (32, 4, 4, 64, 64), "two image groups, input gradient", yx=True, res=True, split=True, multi=True),
    R(_c2(4), "wino", (8, 8, 8, 64, 64), "two image groups at 8x8: tile_fastest on", bias=True, split=True, multi=True),
    R(_c2(8), "wino", (1, 32, 32, 64, 64), "2 x 2 tile blocks per image", bias=True, res=True, split=True),
    R(_c2(8), "wino", (1, 32, 32, 64, 64), "2 x 2 tile blocks, input gradient", family="offset", yx=True, split=True),
    R(_c2(8), "wino", (1, 16, 32, 64, 64), "non-square power-of-two map: 1 x 2 tile blocks", bias=True, split=True),
    R(_c2(8), "wino", (1, 16, 32, 64, 64), "non-square map, input gradient", yx=True, res=True, split=True),
    R(_c2(8), "wino", (2, 16, 16, 64, 64), "two images = two units of one image: the neighbouring image is the next unit",
      family="offset", bias=True, split=True, multi=True),
]
# ---- F(4x4) on 32-tile workgroups (winograd4.hip, lgm_wino4_set_light(0)).  unit_class: 0 = H % 16 == 0 and W % 32 == 0 (one
#      image), 1 = 16x16 (2 images), 2 = 8x8 (8 images), 3 = 4x4 (32 images).  Form::splits: C = 32 (4 phases) is unsplit
#      (min 4 phases per split), C = 64 gives two splits of four phases, C = 192 three splits of 8.
LEDGER += [
    R(_c4(0), "wino4", (1, 16, 32, 32, 64), "smallest class-0 map, 4 phases: unsplit; forward only (32 input channels)", bias=True,
      res=True, split=False),
    R(_c4(0), "wino4", (1, 16, 32, 64, 64), "two splits of four phases", family="offset", bias=True, res=True, split=True),
    R(_c4(0), "wino4", (1, 16, 32, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True),
    R(_c4(0), "wino4", (1, 16, 32, 64, 64), "tile-edge impulses", family="impulse", bias=True, split=True),
    R(_c4(0), "wino4", (1, 16, 32, 64, 64), "tile-edge impulses through the mirrored taps", family="impulse", yx=True, split=True),
    R(_c4(0), "wino4", (1, 48, 32, 64, 64), "tb_h = 3: 6 units, no multiple of 8, so xcd_ranges falls back to unit = blockIdx",
      bias=True, split=True),
    R(_c4(0), "wino4", (1, 48, 32, 64, 64), "tb_h = 3, input gradient", yx=True, split=True),
    R(_c4(0), "wino4", (1, 32, 64, 64, 128), "grid a multiple of 8 with two channel blocks (tn_slowest = 1)", bias=True, res=True,
      split=True),
    R(_c4(0), "wino4", (1, 32, 64, 128, 64), "input gradient, 16 phases", yx=True, res=True, split=True),
    R(_c4(0), "wino4", (14, 32, 64, 32, 128), "tn_slowest = 0: two channel blocks and M = 28672 >= 210 N pixels", bias=True,
      split=False),
    R(_c4(0), "wino4", (1, 16, 32, 192, 64), "24 phases: six splits of four (channel counts are multiples of 32, so the four-phase "
      "minimum divides them: no ragged split below the cap of 16 splits)", bias=True, split=True, planned=6),
    R(_c4(0), "wino4", (1, 16, 32, 544, 64), "68 phases, 16 splits planned: 5 phases each makes 14 splits, the last ragged (3 phases)",
      bias=True, res=True, split=True, planned=16),
    R(_c4(0), "wino4_partial", (1, 16, 32, 64, 64), "the planes stay in the workspace", bias=True, split=True),
    R(_c4(0), "wino4", (1, 16, 32, 64, 64), "unsplit at C = 64", env="LGM_WINO4_SPLITS=1", bias=True, res=True, split=False),
    R(_c4(1), "wino4", (2, 16, 16, 32, 64), "one unit of two images, unsplit", bias=True, split=False, multi=True),
    R(_c4(1), "wino4", (2, 16, 16, 64, 64), "one unit of two images", family="offset", bias=True, res=True, split=True, multi=True),
    R(_c4(1), "wino4", (2, 16, 16, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True, multi=True),
    R(_c4(1), "wino4", (4, 16, 16, 64, 64), "two units", family="impulse", bias=True, split=True, multi=True),
    R(_c4(1), "wino4", (4, 16, 16, 64, 64), "two units, input gradient", family="impulse", yx=True, split=True, multi=True),
    R(_c4(2), "wino4", (8, 8, 8, 32, 64), "one unit of eight images, unsplit", bias=True, split=False, multi=True),
    R(_c4(2), "wino4", (8, 8, 8, 64, 64), "one unit of eight images", family="offset", bias=True, res=True, split=True, multi=True),
    R(_c4(2), "wino4", (8, 8, 8, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True, multi=True),
    R(_c4(2), "wino4", (16, 8, 8, 64, 64), "two units", family="impulse", bias=True, split=True, multi=True),
    R(_c4(2), "wino4", (16, 8, 8, 64, 64), "two units, input gradient", family="impulse", yx=True, split=True, multi=True),
    R(_c4(2), "wino4_partial", (8, 8, 8, 64, 64), "input-gradient planes", yx=True, split=True, multi=True),
    R(_c4(3), "wino4", (32, 4, 4, 32, 64), "one unit of 32 images (one tile each), unsplit", bias=True, split=False, multi=True),
    R(_c4(3), "wino4", (32, 4, 4, 64, 64), "one unit of 32 images", family="offset", bias=True, res=True, split=True, multi=True),
    R(_c4(3), "wino4", (32, 4, 4, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True, multi=True),
    R(_c4(3), "wino4", (64, 4, 4, 128, 64), "two units, 16 phases", family="impulse", bias=True, split=True, multi=True),
    R(_c4(3), "wino4", (64, 4, 4, 64, 128), "two units, input gradient over 16 phases", family="impulse", yx=True, split=True,
      multi=True),
    # ---- the GroupNorm-statistics builds: class-0 maps, unsplit reduction
    R("lgmwino4::wino4_conv_kernel<0, false, 0, true>", "wino4_stats", (1, 16, 32, 32, 64), "smallest class-0 map of the 32-tile "
      "form, 4 phases: unsplit", bias=True, split=False),
    R("lgmwino4l::wino4l_conv_kernel<0, true>", "wino4_stats", (1, 8, 32, 32, 64), "smallest class-0 map of the light form "
      "(8-row units), reached through lgm_conv3x3_wino4_stats under lgm_wino4_set_light(1)", bias=True, split=False, light=1),
    # ---- F(4x4) on light workgroups (winograd4l.hip, its direct entry point): class 0 = H % 8 == 0 and W % 32 == 0, 1 = 16x16
    #      (one image), 2 = 8x8 (four images).  lgm_wino4l_splits: fill the slots while a split keeps >= 4 phases
    R(_l4(0), "wino4l", (1, 8, 32, 32, 64), "smallest class-0 map, unsplit", bias=True, res=True, split=False),
    R(_l4(0), "wino4l", (1, 8, 32, 64, 64), "two splits", family="offset", bias=True, res=True, split=True),
    R(_l4(0), "wino4l", (1, 8, 32, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True),
    R(_l4(0), "wino4l", (1, 8, 32, 64, 64), "tile-edge impulses", family="impulse", bias=True, split=True),
    R(_l4(0), "wino4l", (1, 8, 32, 64, 64), "tile-edge impulses through the mirrored taps", family="impulse", yx=True, split=True),
    R(_l4(0), "wino4l", (1, 24, 64, 64, 64), "3 x 2 units per image", bias=True, split=True),
    R(_l4(0), "wino4l", (1, 8, 32, 544, 64), "68 phases, 16 splits planned: 5 phases each makes 14 splits, the last ragged (3 phases)",
      bias=True, split=True, planned=16),
    R(_l4(0), "wino4l", (1, 24, 64, 32, 64), "3 x 2 units per image, unsplit", res=True, split=False),
    R(_l4(1), "wino4l", (1, 16, 16, 32, 64), "one image per unit, unsplit", bias=True, split=False),
    R(_l4(1), "wino4l", (1, 16, 16, 64, 64), "split", family="offset", bias=True, res=True, split=True),
    R(_l4(1), "wino4l", (1, 16, 16, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True),
    R(_l4(1), "wino4l", (2, 16, 16, 64, 64), "two units, tile-edge impulses", family="impulse", bias=True, split=True),
    R(_l4(1), "wino4l", (2, 16, 16, 64, 64), "two units, tile-edge impulses through the mirrored taps", family="impulse", yx=True,
      split=True),
    R(_l4(2), "wino4l", (4, 8, 8, 32, 64), "one unit of four images, unsplit", bias=True, split=False, multi=True),
    R(_l4(2), "wino4l", (4, 8, 8, 64, 64), "one unit of four images", family="offset", bias=True, res=True, split=True, multi=True),
    R(_l4(2), "wino4l", (4, 8, 8, 64, 64), "input gradient", family="offset", yx=True, res=True, split=True, multi=True),
    R(_l4(2), "wino4l", (8, 8, 8, 64, 64), "two units", family="impulse", bias=True, split=True, multi=True),
    R(_l4(2), "wino4l", (8, 8, 8, 64, 64), "two units, input gradient", family="impulse", yx=True, split=True, multi=True),
]
# ---- F(2x2) weight gradient (winograd.hip) through lgm_conv_wgrad, the only way in.  It takes the Winograd kernel where the
#      direct 3x3 weight gradient's whole image groups hold too (4x4 maps: B % 8, not the B % 4 of wgrad_class alone), so the
#      smallest 4x4 row is B = 8.  wino_wgrad_plan_budget: two chunks per split wherever a round of workgroups is not full.
#      slabs = the slab count the deferred launch reports (desc[6]), asserted.  alt = the geometry of every second layer of a group.
for _G, _geom, _slabs, _why in [(2, (8, 4, 4, 64, 64), 2, "4 chunks: two slabs of two chunks (B = 8: lgm_wgrad3x3_supported wants whole "
                                 "groups of 8 images at 4x4)"),
                                (4, (2, 8, 8, 64, 64), 2, "4 chunks: two slabs of two chunks"),
                                (8, (1, 16, 16, 64, 64), 4, "8 chunks: four slabs of two chunks"),
                                (8, (3, 16, 16, 64, 128), 12, "24 chunks, two blocks: the plan takes 12 slabs of two chunks (no ragged "
                                 "split: below a full round of workgroups the plan always ends at two chunks per slab)"),
                                (8, (34, 16, 16, 64, 128), 91, "272 chunks, two blocks: 128 slabs fill the round, 3 chunks per slab -> "
                                 "91 slabs, the last ragged (2 chunks)")]:
    _n = f"lgmwino::wino_wgrad_kernel<{_G}, false>"
    LEDGER += [
        R(_n, "conv_wgrad", _geom, _why, beta=0.0, gbias=True),
        R(_n, "conv_wgrad", _geom, _why + "; accumulated by the launch's own reducer", beta=1.0, gbias=True),
        R(_n, "conv_wgrad", _geom, _why + "; slabs through wgrad_reduce_batch", beta=0.0, gbias=False, defer=True, slabs=_slabs),
        R(_n, "conv_wgrad", _geom, _why + "; slabs through wgrad_reduce_batch, accumulated", family="offset", beta=1.0, gbias=False,
          defer=True, slabs=_slabs),
    ]
    if _geom[0] <= 8 and _geom[4] == 64:
        _alt = (2 * _geom[0], _geom[1], _geom[2], 64, 128)
        LEDGER += [
            R(_n, "conv_wgrad", _geom, "tile-edge impulses", family="impulse", beta=1.0, gbias=True, defer=True, slabs=_slabs),
            R(f"lgmwino::wino_wgrad2_kernel<{_G}>", "wgradn", _geom, "two layers in one launch", layers=2, alt=_alt),
            R(f"lgmwino::wino_wgrad4_kernel<{_G}>", "wgradn", _geom, "three layers in one launch", family="offset", layers=3, alt=_alt),
            R(f"lgmwino::wino_wgrad4_kernel<{_G}>", "wgradn", _geom, "four layers in one launch", layers=4, alt=_alt),
        ]
LEDGER += [
    R("lgmwino::wino_bwd_pair_kernel<2>", "wino_bwd", (16, 4, 4, 64, 64), "input gradient + weight gradient in one launch", res=True,
      gbias=True, beta=1.0, multi=True),
    R("lgmwino::wino_bwd_pair_kernel<4>", "wino_bwd", (4, 8, 8, 64, 64), "input gradient + weight gradient in one launch",
      gbias=True, beta=0.0, multi=True),
    R("lgmwino::wino_bwd_pair_kernel<8>", "wino_bwd", (1, 16, 16, 64, 64), "input gradient + weight gradient in one launch", res=True,
      gbias=False, beta=1.0),
]
# ---- F(4x4) weight gradient (winograd4_wgrad.hip): groups of 64 pixels; sq = 0 row groups (W % 16 == 0), 1 square groups
#      (W % 16 != 0), 2 image groups (4x4 maps, four images)
_W4 = "lgmwino4w::wino4_wgrad_kernel"
LEDGER += [
    R(_W4, "wino4_wgrad", (1, 16, 16, 32, 64), "row groups, 4 groups: two slabs of two", beta=0.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (1, 16, 16, 32, 64), "row groups, accumulated", family="offset", beta=1.0, gbias=False, slabs=2),
    R(_W4, "wino4_wgrad", (1, 16, 16, 32, 64), "row groups, tile-edge impulses", family="impulse", beta=0.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (1, 4, 64, 32, 64), "row groups with H = 4: one tile row", beta=0.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (4, 8, 8, 32, 64), "square groups (W = 8)", beta=1.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (4, 8, 8, 32, 64), "square groups, tile-edge impulses", family="impulse", beta=0.0, gbias=False, slabs=2),
    R(_W4, "wino4_wgrad", (2, 8, 24, 32, 64), "square groups with grow = 3: 6 groups, three slabs of two", family="offset", beta=0.0,
      gbias=True, slabs=3),
    R(_W4, "wino4_wgrad", (5, 8, 8, 64, 64), "5 groups: two slabs of 3 and 2, the last ragged", beta=1.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (16, 4, 4, 32, 64), "image groups", beta=0.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (16, 4, 4, 32, 64), "image groups, accumulated", family="offset", beta=1.0, gbias=False, slabs=2),
    R(_W4, "wino4_wgrad", (16, 4, 4, 32, 64), "image groups, tile-edge impulses", family="impulse", beta=1.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (4, 8, 8, 32, 64), "the other unit order", env="LGM_W4W_XCD=0", beta=0.0, gbias=True, slabs=2),
    R(_W4, "wino4_wgrad", (1, 16, 16, 32, 64), "the other unit order, row groups", env="LGM_W4W_XCD=0", beta=1.0, gbias=True, slabs=2),
]
# the grouped launch takes the F(4x4) kernel only where lgm_wino4_wgrad_use says so (the layer's F(4x4) input gradient is
# preferred): 16x16 maps under light workgroups from 32 units of 32 tiles, B = 64 - the smallest batch that reaches it
_GW = (64, 16, 16, 64, 128)
LEDGER += [
    R("lgmwino4w::wino4_wgrad2_kernel", "wgradn", _GW, "two layers in one F(4x4) launch", layers=2, light=1, alt=(64, 16, 16, 128, 128)),
    R("lgmwino4w::wino4_wgrad4_kernel", "wgradn", _GW, "three layers", layers=3, light=1, alt=(64, 16, 16, 128, 128)),
    R("lgmwino4w::wino4_wgrad4_kernel", "wgradn", _GW, "four layers", family="offset", layers=4, light=1),
    R("lgmwino4w::wino4_wgrad8_kernel", "wgradn", _GW, "five layers", layers=5, light=1),
    R("lgmwino4w::wino4_wgrad8_kernel", "wgradn", _GW, "eight layers", layers=8, light=1),
]


def row_id(row):
    o = row["opts"]
    tags = [o["family"]] + [k for k in ("yx", "bias", "res", "gbias", "defer") if o.get(k)]
    tags += [f"{k}{o[k]:g}" for k in ("beta", "layers", "light") if k in o]
    return f"{row['name']}|{row['entry']}|{'x'.join(map(str, row['geom']))}|{','.join(tags)}" + (f"|{row['env']}" if row["env"] else "")


def transform_of(row):
    return 2 if row["name"].startswith("lgmwino::") else 4


def kind_of(row):
    return "wgrad" if row["entry"] in ("conv_wgrad", "wgradn", "wino4_wgrad") else "yx" if row["opts"].get("yx") else "xy"


def families_of(row):
    """the row's own family, and all-images-zero-but-one where its unit packs several images"""
    fams = [row["opts"]["family"]]
    if row["opts"].get("multi") and kind_of(row) != "wgrad":
        fams.append("one_live_image")
    return fams


_PROBLEMS = {}


def problem(row, family=None, kind=None, beta=None, geom=None, seed=None):
    """the oracle's Problem of one row (cached: the float64 reference and S_W are computed once)"""
    o = row["opts"]
    family = family or o["family"]
    kind = kind or kind_of(row)
    geom = geom or row["geom"]
    live = family == "one_live_image"
    beta = o.get("beta", 0.0) if beta is None else beta
    key = (kind, transform_of(row), geom, family, bool(o.get("bias")) and not live, bool(o.get("res")) and not live, beta, seed)
    if key not in _PROBLEMS:
        if len(_PROBLEMS) > 12:
            _PROBLEMS.clear()
        _PROBLEMS[key] = OW.Problem(kind, key[1], geom, family, bias=key[4], res=key[5], beta=beta if kind == "wgrad" else 0.0, seed=seed)
    return _PROBLEMS[key]


def layers_of(row):
    """(geometry, Problem) of every layer of a grouped weight-gradient row: every layer its own inputs, every second one the
    row's other geometry, beta alternating"""
    o = row["opts"]
    geoms = [row["geom"] if k % 2 == 0 else o.get("alt", row["geom"]) for k in range(o["layers"])]
    return [(g, problem(row, beta=float(k % 2), geom=g, seed=1000 + 17 * k + sum(g))) for k, g in enumerate(geoms)]


def registry_names():
    from lgm_hip import _lib
    D = _lib.lib()._dll
    D.lgm_kernel_name.restype = ctypes.c_char_p
    return sorted({D.lgm_kernel_name(i).decode() for i in range(D.lgm_kernel_name_count())})


# ---- completeness and plans (no GPU) --------------------------------------------------------------------------------------
def test_every_winograd_kernel_name_has_a_ledger_row():
    names = [n for n in registry_names() if n.startswith(PREFIXES)]
    keys = {r["name"] for r in LEDGER}
    assert len(names) >= 28
    assert sorted(set(names) - keys) == [], "registry names of the Winograd files without a ledger row"
    assert sorted(keys - set(names)) == [], "ledger rows whose name the library can never note"
    assert len({row_id(r) for r in LEDGER}) == len(LEDGER)
    for r in LEDGER:
        assert r["opts"]["family"] in OW.FAMILIES and len(r["geom"]) == 5
    # every name gets `plain`; offset and impulse once per (file, direction, unit class)
    for n in names:
        assert any(r["name"] == n and r["opts"]["family"] == "plain" for r in LEDGER), n
    for fam in ("offset", "impulse"):
        for n in names:
            if "wgrad2" in n or "wgrad4" in n or "wgrad8" in n or "bwd_pair" in n or ", true>" in n:
                continue                      # the grouped / pair / statistics launches run the same device code as the single ones
            kinds = {kind_of(r) for r in LEDGER if r["name"] == n}
            for k in kinds:
                assert any(r["name"] == n and kind_of(r) == k and r["opts"]["family"] == fam for r in LEDGER), (n, k, fam)


def _light(L, row):
    L.lgm_wino4_set_light(row["opts"].get("light", 0))
    from lgm_hip import ops
    ops.clear_plan_caches()


def test_rows_reach_the_plans_they_name():
    """The library's own *_supported / *_workspace answers for every row that runs without an environment switch: the entry
    point takes the geometry, and the reduction is split exactly where the row says so."""
    from lgm_hip import ops
    L = ops.lib()
    try:
        for row in LEDGER:
            if row["env"]:
                continue
            B, H, W, Cin, Cout = row["geom"]
            g = ops.make_geom(B, H, W, Cin, Cout, 3, 3, 1, 1)
            o, e = row["opts"], row["entry"]
            yx = 1 if o.get("yx") else 0
            _light(L, row)
            if e in ("wino", "wino_partial"):
                assert L.lgm_conv3x3_wino_supported(ctypes.byref(g), yx) == 1, row_id(row)
                ws = (L.lgm_conv3x3_wino_workspace if e == "wino" else L.lgm_conv3x3_wino_workspace_partial)(ctypes.byref(g), yx)
                assert (ws > 0) == o["split"], (row_id(row), ws)
                assert "planned" not in o or ws == o["planned"] * B * H * W * (Cin if yx else Cout) * 4, (row_id(row), ws)
            elif e in ("wino4", "wino4_partial", "wino4_stats"):
                assert L.lgm_conv3x3_wino4_supported(ctypes.byref(g), yx) == 1, row_id(row)
                ws = L.lgm_conv3x3_wino4_workspace(ctypes.byref(g), yx)
                assert (ws > 0) == o["split"], row_id(row)
                assert "planned" not in o or ws == o["planned"] * B * H * W * (Cin if yx else Cout) * 4, (row_id(row), ws)
                if e == "wino4_stats":
                    per = ctypes.c_int(0)
                    assert L.lgm_conv3x3_wino4_stats_floats(ctypes.byref(g), ctypes.addressof(per)) == B * per.value * 2 * Cout > 0
            elif e == "wino4l":
                assert L.lgm_conv3x3_wino4l_supported(ctypes.byref(g), yx) == 1, row_id(row)
                ws = L.lgm_conv3x3_wino4l_workspace(ctypes.byref(g), yx)
                assert (ws > 0) == o["split"], row_id(row)
                assert "planned" not in o or ws == o["planned"] * B * H * W * (Cin if yx else Cout) * 4, (row_id(row), ws)
            elif e == "wino4_wgrad":
                assert L.lgm_conv3x3_wino4_wgrad_supported(ctypes.byref(g)) == 1, row_id(row)
                assert L.lgm_conv3x3_wino4_wgrad_workspace(ctypes.byref(g)) == o["slabs"] * (Cout * 9 * Cin + Cout) * 4, row_id(row)
            elif e == "wgradn":
                gs = [ops.make_geom(*gg, 3, 3, 1, 1) for gg in [row["geom"], o.get("alt", row["geom"])] * 4][:o["layers"]]
                assert ops.wgrad_group_supported(gs), row_id(row)
                for gg in gs:
                    assert (L.lgm_conv3x3_wino4_preferred(ctypes.byref(gg), 1) == 1) == row["name"].startswith("lgmwino4w::"), row_id(row)
            elif e == "wino_bwd":
                assert L.lgm_conv3x3_wino_bwd_supported(ctypes.byref(g), Cout + 8, Cin + 8, Cin + 8, Cin + 8) == 1, row_id(row)
            elif e == "conv_wgrad":
                assert L.lgm_conv3x3_wino4_preferred(ctypes.byref(g), 1) == 0, row_id(row)
    finally:
        L.lgm_wino4_set_light(-1)
        ops.clear_plan_caches()


# ---- operands -----------------------------------------------------------------------------------------------------------
LO, HI = 4, 12          # floats of NaN before / after the channel slice of every pixel (16-byte aligned slices)


def _slice(dev, B, H, W, C, src=None):
    """A [B, H, W, C] channel slice of a wider NaN-filled allocation: NaN in the channels beside it, in one full image row before
    the first pixel and in one after the last.  ``src``: NCHW cpu tensor to put there (else the slice is NaN too)."""
    P = C + LO + HI
    buf = torch.full(((B * H + 2) * W, P), NAN, device=dev)
    view = buf[W:W + B * H * W].view(B, H, W, P)[..., LO:LO + C]
    if src is not None:
        view.copy_(src.permute(0, 2, 3, 1).to(dev))
    return view, buf


def _slice_intact(view, buf):
    """nothing but the slice itself was written: every float around it is still NaN"""
    B, H, W, C = view.shape
    probe = buf.clone()
    probe[W:W + B * H * W, LO:LO + C] = NAN
    return bool(torch.isnan(probe).all())


def _flat(dev, n, fill):
    buf = torch.full((n + 64,), NAN, device=dev)
    view = buf[32:32 + n]
    if isinstance(fill, torch.Tensor):
        view.copy_(fill.reshape(-1).to(dev))
    else:
        view.fill_(fill)
    return view, buf


def _flat_intact(buf, n):
    return bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[32 + n:]).all())


def _nchw(view):
    return view.detach().cpu().permute(0, 3, 1, 2)


def _host_u2(w):
    """The F(2x2) operand Uf[n/32][c/8][xi][(c%8)/4][n%32][c%4] = (G g G^T)[xi] of forward-form weights w [N, C, 3, 3], in
    float32 on the host: for channel counts lgm_wino_weights' 32 x 32 blocks do not cover."""
    N, C = w.shape[:2]
    U = OW.transform_w(w.float(), 2).reshape(N // 32, 32, C // 8, 2, 4, 16)           # [nb][n][chunk][kh][c4][xi]
    return U.permute(0, 2, 5, 3, 1, 4).contiguous().reshape(-1)


def _weights(row, pr, dev):
    """the transformed weight operand of the row's direction, written by the library's own transform kernels"""
    from lgm_hip import ops
    m, yx = transform_of(row), kind_of(row) == "yx" or row["entry"] == "wino_bwd"
    w = pr.t["w"]
    N, C = w.shape[:2]
    if m == 2 and (N % 32 or C % 32):
        u = _host_u2(OW.mirrored(w) if yx else w)
        buf = torch.full((u.numel() + 16384,), NAN, device=dev)     # NaN behind it: the weight ring's look-ahead must not be used
        buf[:u.numel()] = u.to(dev)
        return buf
    wd = w.permute(0, 2, 3, 1).reshape(N, 9, C).contiguous().to(dev)
    t2 = m + 2
    # (NaN behind both operands: the weight ring's look-ahead past the last phase must not be used)
    uf = torch.full((N * C * t2 * t2 + 16384,), NAN, device=dev)
    ub = torch.full((N * C * t2 * t2 + 16384,), NAN, device=dev) if (m == 2 or C % 64 == 0) else None
    tab = torch.tensor([[0, N, C, 0, 0, 0]], dtype=torch.int64, device=dev)
    f = ops.lib().lgm_wino_weights if m == 2 else ops.lib().lgm_wino4_weights
    f(wd.data_ptr(), uf.data_ptr(), None if ub is None else ub.data_ptr(), tab.data_ptr(), 1, (N // 32) * (C // 32), ops.stream())
    return ub if yx else uf


def _last():
    from lgm_hip import ops
    k = ops.lib()._dll.lgm_last_kernel()
    return k.decode() if k else ""


def _check(out, what, score, tol):
    out["checks"].append({"what": what, "score": score, "tol": tol})


# ---- forward / input gradient -------------------------------------------------------------------------------------------
def _run_conv(row, dev, out):
    from lgm_hip import ops
    L = ops.lib()
    B, H, W, Cin, Cout = row["geom"]
    o, e = row["opts"], row["entry"]
    yx = 1 if o.get("yx") else 0
    gc, oc = (Cout, Cin) if yx else (Cin, Cout)
    g = ops.make_geom(B, H, W, Cin, Cout, 3, 3, 1, 1)
    _light(L, row)
    out["name"], out["guards"], out["deterministic"] = None, True, True
    for family in families_of(row):
        pr = problem(row, family)
        t = pr.t
        a, _ = _slice(dev, B, H, W, gc, t["gy"] if yx else t["x"])
        u = _weights(row, pr, dev)
        bd = t["bx" if yx else "b"].to(dev) if pr.bias else None
        rd = _slice(dev, B, H, W, oc, t["res_x" if yx else "res_y"])[0] if pr.res else None
        bp = None if bd is None else bd.data_ptr()
        rp, rpitch = (None, 0) if rd is None else (rd.data_ptr(), ops.pitch(rd))
        results = []
        for rep in range(2):
            y, ybuf = _slice(dev, B, H, W, oc)
            if e in ("wino", "wino4", "wino4l"):
                wsf = {"wino": L.lgm_conv3x3_wino_workspace, "wino4": L.lgm_conv3x3_wino4_workspace,
                       "wino4l": L.lgm_conv3x3_wino4l_workspace}[e]
                n = wsf(ctypes.byref(g), yx)
                if row["env"] is None:
                    assert (n > 0) == o["split"], (row_id(row), n)
                ws = torch.full((n // 4 + 16,), NAN, device=dev) if n > 0 else None
                f = {"wino": L.lgm_conv3x3_wino, "wino4": L.lgm_conv3x3_wino4, "wino4l": L.lgm_conv3x3_wino4l}[e]
                f(yx, ctypes.byref(g), a.data_ptr(), ops.pitch(a), u.data_ptr(), bp, rp, rpitch, y.data_ptr(), ops.pitch(y),
                  None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, ops.stream())
                name = _last()
                got = y
            elif e in ("wino_partial", "wino4_partial"):
                n = (L.lgm_conv3x3_wino_workspace_partial if e == "wino_partial" else L.lgm_conv3x3_wino4_workspace)(ctypes.byref(g), yx)
                ws = torch.full((max(n // 4, 4) + 16,), NAN, device=dev)
                part = (ctypes.c_int64 * 2)()
                f = L.lgm_conv3x3_wino_partial if e == "wino_partial" else L.lgm_conv3x3_wino4_partial
                f(yx, ctypes.byref(g), a.data_ptr(), ops.pitch(a), u.data_ptr(), bp, y.data_ptr(), ops.pitch(y), ws.data_ptr(),
                  ws.numel() * 4, ctypes.addressof(part), ops.stream())
                name = _last()
                planes, stride = int(part[0]), int(part[1])
                assert planes > 1, f"{row_id(row)}: the partial form was expected to leave planes"
                assert bool(torch.isnan(y).all()), "the partial form must leave `out` alone"
                acc = ws[:stride].clone()                     # the reducer's order: plane 0, 1, ..., then the bias
                for k in range(1, planes):
                    acc = acc + ws[k * stride:(k + 1) * stride]
                got = acc.view(B, H, W, oc)
                if bd is not None:
                    got = got + bd
                out["guards"] = out["guards"] and bool(torch.isnan(ws[planes * stride:]).all())
            else:                                             # wino4_stats
                per = ctypes.c_int(0)
                n = L.lgm_conv3x3_wino4_stats_floats(ctypes.byref(g), ctypes.addressof(per))
                assert n == B * per.value * 2 * oc > 0, row_id(row)
                st, stbuf = _flat(dev, n, NAN)
                L.lgm_conv3x3_wino4_stats(ctypes.byref(g), a.data_ptr(), ops.pitch(a), u.data_ptr(), bp, y.data_ptr(), ops.pitch(y),
                                          st.data_ptr(), n, ops.stream())
                name = _last()
                got = y
                out["guards"] = out["guards"] and _flat_intact(stbuf, n)
                results.append(st.clone())
            torch.cuda.synchronize()
            out["name"] = name if out["name"] in (None, name) else f"{out['name']} then {name}"
            out["guards"] = out["guards"] and _slice_intact(y, ybuf)
            results.append(got.clone())
        k = len(results) // 2
        out["deterministic"] = out["deterministic"] and all(torch.equal(p, q) for p, q in zip(results[:k], results[k:]))
        _check(out, f"{'input gradient' if yx else 'forward'} [{family}]", pr.score(_nchw(results[-1])), pr.tolerance())
        if e == "wino4_stats":
            _score_stats(out, row, pr, results[-2], results[-1], per.value)


# statistics row `part` of a unit -> its share (tile-row half, output row pair).  Both forms write row `wave` (32-tile form:
# the wave within its half of the workgroup, part = (tid >> 6) & 3; light form: wid) and give wave w the tiles of tile-row half
# w & 1 (et = 16 (w & 1) + lane / 4, resp. 8 (w & 1) + lane / 8) and the output row pair w >> 1 (rpair = tid >> 7).
PART_SHARE = [(0, 0), (1, 0), (0, 1), (1, 1)]


def _score_stats(out, row, pr, st, y, per):
    """The statistics rows [spatial unit][4 parts][2: sum y, sum y^2][N] of the PRE-BIAS outputs against float64 sums of the y this
    launch wrote, row by row.  A row is one wave's share of its unit: half of the unit's tile rows (32-tile form: two of four,
    light form: one of two) x one pair of output rows of every tile (rows 0 and 2, or 1 and 3) - n = 128 / 64 elements - in the
    order the kernels fix (PART_SHARE)."""
    B, H, W, Cin, Cout = row["geom"]
    uh = 8 if row["opts"].get("light") else 16
    units = B * (H // uh) * (W // 32)
    assert per == (H // uh) * (W // 32) * 4
    rows = st.double().cpu().view(units, 4, 2, Cout)
    pre = y.double().cpu() - (pr.t["b"].double() if pr.bias else 0.0)                      # [B, H, W, N]
    pu = pre.view(B, H // uh, uh, W // 32, 32, Cout).permute(0, 1, 3, 2, 4, 5).reshape(units, uh, 32, Cout)
    r = torch.arange(uh)
    parts = torch.stack([pu[:, (r // (uh // 2) == half) & ((r % 4) % 2 == pair)].reshape(units, -1, Cout)
                         for half, pair in PART_SHARE], 1)                                 # [units][4][n][N]
    n = parts.shape[2]
    assert n == uh * 32 // 4
    s1, a1, s2 = parts.sum(2), parts.abs().sum(2), (parts * parts).sum(2)
    _check(out, "statistics rows: sum y", bounds.forward_error_units(rows[:, :, 0], s1, a1), bounds.tolerance(n))
    _check(out, "statistics rows: sum y^2", bounds.forward_error_units(rows[:, :, 1], s2, s2), bounds.tolerance(n))


# ---- weight gradients -----------------------------------------------------------------------------------------------------
def _wgrad_operands(pr, dev, row):
    B, H, W, Cin, Cout = row["geom"]
    gy, _ = _slice(dev, B, H, W, Cout, pr.t["gy"])
    x, _ = _slice(dev, B, H, W, Cin, pr.t["x"])
    return gy, x


def _phys64(t):
    N, C = t.shape[:2]
    return t.permute(0, 2, 3, 1).reshape(N, 9, C)


def _score_wgrad(out, tag, pr, gw, gb):
    N, C = pr.ref.shape[:2]
    got = gw.detach().cpu().view(N, 9, C).view(N, 3, 3, C).permute(0, 3, 1, 2)
    _check(out, f"{tag} gw [{pr.family}]", pr.score(got), pr.tolerance())
    if gb is not None:
        _check(out, f"{tag} fused bias gradient [{pr.family}]", bounds.forward_error_units(gb, pr.ref_b, pr.S_b),
               bounds.tolerance(pr.n_bias))


def _wgrad_outputs(pr, dev, gbias):
    N, C = pr.ref.shape[:2]
    gw0 = _phys64(pr.t["gw0"]) if pr.beta else NAN
    gw, wbuf = _flat(dev, N * 9 * C, gw0)
    gb, bbuf = _flat(dev, N, pr.t["gb0"] if pr.beta else NAN) if gbias else (None, None)
    return gw, wbuf, gb, bbuf


def _nan_ws(dev, nbytes):
    """a slab workspace of the launch's own, all NaN: what the launch does not write shows in the reduced gradient"""
    return torch.full((nbytes // 4 + 16,), NAN, device=dev)


def _run_wgrad(row, dev, out):
    """one layer: lgm_conv_wgrad (the F(2x2) kernel, reduced by the launch itself), lgm_conv_wgrad_deferred (its slabs through
    wgrad_reduce_batch) or lgm_conv3x3_wino4_wgrad (slabs only)"""
    from lgm_hip import ops
    L = ops.lib()
    B, H, W, Cin, Cout = row["geom"]
    o = row["opts"]
    g = ops.make_geom(B, H, W, Cin, Cout, 3, 3, 1, 1)
    _light(L, row)
    pr = problem(row)
    gy, x = _wgrad_operands(pr, dev, row)
    results, out["guards"] = [], True
    for rep in range(2):
        gw, wbuf, gb, bbuf = _wgrad_outputs(pr, dev, o["gbias"])
        gbp = None if gb is None else gb.data_ptr()
        desc = (ctypes.c_int64 * 8)()
        if row["entry"] == "wino4_wgrad":
            ws = _nan_ws(dev, L.lgm_conv3x3_wino4_wgrad_workspace(ctypes.byref(g)))
            L.lgm_conv3x3_wino4_wgrad(ctypes.byref(g), gy.data_ptr(), ops.pitch(gy), x.data_ptr(), ops.pitch(x), gw.data_ptr(), gbp,
                                      pr.beta, ws.data_ptr(), ws.numel() * 4, ctypes.addressof(desc), ops.stream())
            out["name"] = _last()
        elif o.get("defer"):
            ws = _nan_ws(dev, L.lgm_conv_wgrad_workspace(ctypes.byref(g)))
            L.lgm_conv_wgrad_deferred(ctypes.byref(g), gy.data_ptr(), ops.pitch(gy), x.data_ptr(), ops.pitch(x), gw.data_ptr(), gbp,
                                      pr.beta, ws.data_ptr(), ws.numel() * 4, ctypes.addressof(desc), ops.stream())
            out["name"] = _last()
        else:
            ws = _nan_ws(dev, L.lgm_conv_wgrad_workspace(ctypes.byref(g)))
            L.lgm_conv_wgrad(ctypes.byref(g), gy.data_ptr(), ops.pitch(gy), x.data_ptr(), ops.pitch(x), gw.data_ptr(), gbp, pr.beta,
                             ws.data_ptr(), ws.numel() * 4, ops.stream())
            out["name"] = _last()
        if row["entry"] == "wino4_wgrad" or o.get("defer"):
            assert desc[0] == ws.data_ptr() and desc[6] == o["slabs"], f"{row_id(row)}: {desc[6]} slabs ({row['why']})"
            ops.wgrad_reduce_batch([tuple(desc)], dev)
        torch.cuda.synchronize()
        out["guards"] = out["guards"] and _flat_intact(wbuf, gw.numel()) and (gb is None or _flat_intact(bbuf, gb.numel()))
        results.append((gw.clone(), None if gb is None else gb.clone()))
    _score_wgrad(out, "beta = %g" % pr.beta, pr, *results[0])
    out["deterministic"] = bool(torch.equal(results[0][0], results[1][0])) and \
        (results[0][1] is None or bool(torch.equal(results[0][1], results[1][1])))


def _run_wgradn(row, dev, out):
    """``layers`` layers in ONE launch (lgm_conv3x3_wino_wgradn): every layer its own inputs, every second one the row's other
    geometry, beta and the fused bias gradient alternating; every layer scored on its own, against its own S_W"""
    from lgm_hip import ops
    L = ops.lib()
    _light(L, row)
    layers = layers_of(row)
    n = len(layers)
    geoms = [ops.make_geom(*gg, 3, 3, 1, 1) for gg, _ in layers]
    arr = (ctypes.c_void_p * n)(*[ctypes.addressof(g) for g in geoms])
    assert L.lgm_conv3x3_wino_wgradn_supported(n, ctypes.addressof(arr)) == 1, row_id(row)
    need = (ctypes.c_int64 * n)()
    L.lgm_conv3x3_wino_wgradn_workspaces(n, ctypes.addressof(arr), ctypes.addressof(need))
    operands = []
    for gg, pr in layers:
        B, H, W, Cin, Cout = gg
        operands.append((_slice(dev, B, H, W, Cout, pr.t["gy"])[0], _slice(dev, B, H, W, Cin, pr.t["x"])[0]))
    results, out["guards"] = [], True
    for rep in range(2):
        outs = [_wgrad_outputs(pr, dev, k % 3 != 2) for k, (_, pr) in enumerate(layers)]
        wss = [_nan_ws(dev, int(need[k])) for k in range(n)]
        descs = [(ctypes.c_int64 * 8)() for _ in range(n)]
        items = (ops.WgradItem * n)()
        for k, (_, pr) in enumerate(layers):
            gy, x = operands[k]
            gw, _, gb, _ = outs[k]
            items[k] = ops.WgradItem(ctypes.addressof(geoms[k]), gy.data_ptr(), ops.pitch(gy), x.data_ptr(), ops.pitch(x), gw.data_ptr(),
                                     None if gb is None else gb.data_ptr(), pr.beta, wss[k].data_ptr(), wss[k].numel() * 4,
                                     ctypes.addressof(descs[k]))
        L.lgm_conv3x3_wino_wgradn(n, ctypes.addressof(items), ops.stream())
        out["name"] = _last()
        assert all(d[6] >= 2 and d[0] == ws.data_ptr() and d[6] * d[1] * 4 <= need[k] for k, (d, ws) in enumerate(zip(descs, wss)))
        ops.wgrad_reduce_batch([tuple(d) for d in descs], dev)
        torch.cuda.synchronize()
        for gw, wbuf, gb, bbuf in outs:
            out["guards"] = out["guards"] and _flat_intact(wbuf, gw.numel()) and (gb is None or _flat_intact(bbuf, gb.numel()))
        results.append([(gw.clone(), None if gb is None else gb.clone()) for gw, _, gb, _ in outs])
    for k, (gg, pr) in enumerate(layers):
        _score_wgrad(out, f"layer {k} of {n} ({'x'.join(map(str, gg))}), beta = {k % 2}", pr, *results[0][k])
    out["deterministic"] = all(torch.equal(p[0], q[0]) and (p[1] is None or torch.equal(p[1], q[1])) for p, q in zip(*results))


def _run_bwd_pair(row, dev, out):
    """lgm_conv3x3_wino_bwd: the input gradient and the weight gradient of one layer in one launch; where its unit packs
    several images, a second time with all images zero but one and no residual"""
    from lgm_hip import ops
    L = ops.lib()
    B, H, W, Cin, Cout = row["geom"]
    o = row["opts"]
    g = ops.make_geom(B, H, W, Cin, Cout, 3, 3, 1, 1)
    _light(L, row)
    two = (ctypes.c_int64 * 2)()
    L.lgm_conv3x3_wino_bwd_workspaces(ctypes.byref(g), 0, ctypes.addressof(two))
    out["guards"], out["deterministic"] = True, True
    for family in families_of(row):
        pw = problem(row, family, kind="wgrad")
        py = problem(row, family, kind="yx")
        assert all(torch.equal(pw.t[k], py.t[k]) for k in ("x", "gy", "w"))
        gy, x = _wgrad_operands(pw, dev, row)
        ub = _weights(row, py, dev)
        rd = _slice(dev, B, H, W, Cin, py.t["res_x"])[0] if py.res else None
        results = []
        for rep in range(2):
            gx, xbuf = _slice(dev, B, H, W, Cin)
            gw, wbuf, gb, bbuf = _wgrad_outputs(pw, dev, o["gbias"])
            dws = torch.full((max(two[0] // 4, 4) + 16,), NAN, device=dev)
            wws = _nan_ws(dev, two[1])
            L.lgm_conv3x3_wino_bwd(ctypes.byref(g), gy.data_ptr(), ops.pitch(gy), x.data_ptr(), ops.pitch(x), ub.data_ptr(),
                                   None if rd is None else rd.data_ptr(), 0 if rd is None else ops.pitch(rd), gx.data_ptr(), ops.pitch(gx),
                                   dws.data_ptr(), dws.numel() * 4, None, gw.data_ptr(), None if gb is None else gb.data_ptr(), pw.beta,
                                   wws.data_ptr(), wws.numel() * 4, None, ops.stream())
            name = _last()
            out["name"] = name if out["name"] in (None, name) else f"{out['name']} then {name}"
            torch.cuda.synchronize()
            out["guards"] = out["guards"] and _slice_intact(gx, xbuf) and _flat_intact(wbuf, gw.numel()) and \
                (gb is None or _flat_intact(bbuf, gb.numel()))
            results.append((gx.clone(), gw.clone(), None if gb is None else gb.clone()))
        _check(out, f"input gradient [{family}]", py.score(_nchw(results[0][0])), py.tolerance())
        _score_wgrad(out, "beta = %g" % pw.beta, pw, results[0][1], results[0][2])
        out["deterministic"] = out["deterministic"] and all(p is None or torch.equal(p, q) for p, q in zip(*results))


RUNNERS = {"wino": _run_conv, "wino_partial": _run_conv, "wino4": _run_conv, "wino4l": _run_conv, "wino4_partial": _run_conv,
           "wino4_stats": _run_conv, "conv_wgrad": _run_wgrad, "wino4_wgrad": _run_wgrad, "wgradn": _run_wgradn,
           "wino_bwd": _run_bwd_pair}


def run_row(row, dev):
    out = {"row": row_id(row), "name": None, "checks": [], "guards": None, "deterministic": None}
    from lgm_hip import ops
    try:
        RUNNERS[row["entry"]](row, dev, out)
    finally:                                   # whatever the row did: the files that run after this one see the defaults
        ops.lib().lgm_wino4_set_light(-1)
        ops.clear_plan_caches()
    return out


def judge(row, out, parity):
    """The assertions of one row, from the record its run left (in this process or in a child)."""
    assert out["name"] == row["name"], f"{row_id(row)}: ran {out['name']!r} ({row['why']})"
    assert out["checks"]
    for c in out["checks"]:
        parity(f"{row_id(row)} {c['what']} [units of 2^-24 S_W]", c["score"], c["tol"])
    assert out["guards"] is True, f"{row_id(row)}: a NaN guard around an output was written"
    assert out["deterministic"] is True, f"{row_id(row)}: two launches differ"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


_GPU_ERROR = []


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in LEDGER if r["env"] is None], ids=row_id)
def test_ledger_row(dev, parity, row):
    assert not _GPU_ERROR, f"the runtime reported an error at {_GPU_ERROR[0]}: nothing more is launched in this session"
    try:
        out = run_row(row, dev)
    except RuntimeError as exc:                      # a HIP error is sticky: later launches would only repeat it
        if "hip" in str(exc).lower():
            _GPU_ERROR.append(row_id(row))
        raise
    judge(row, out, parity)


SWITCHES = sorted({r["env"] for r in LEDGER if r["env"]})
_CHILD_DIED = []


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
def test_switch_rows(parity, switch):
    """every row of one environment switch in a fresh child process (the library reads a switch once per process)"""
    assert not _CHILD_DIED, f"an earlier child died ({_CHILD_DIED[0]}): no further child is started in this session"
    assert not _GPU_ERROR, f"the runtime reported an error at {_GPU_ERROR[0]}: no child is started in this session"
    rows = [r for r in LEDGER if r["env"] == switch]
    env = dict(os.environ)
    key, val = switch.split("=")
    env[key] = val
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", switch], env=env, capture_output=True,
                             text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(f"{switch}: timeout")
        raise
    if res.returncode != 0:
        _CHILD_DIED.append(f"{switch}: exit status {res.returncode}")
    assert res.returncode == 0, res.stderr[-2000:]
    outs = {o["row"]: o for o in json.loads(res.stdout.strip().splitlines()[-1])}
    assert sorted(outs) == sorted(row_id(r) for r in rows)
    for r in rows:
        judge(r, outs[row_id(r)], parity)


def _child(switch):
    key, val = switch.split("=")
    assert os.environ.get(key) == val
    dev = torch.device("cuda", 0)
    outs = [run_row(r, dev) for r in LEDGER if r["env"] == switch]
    for o in outs:
        for c in o["checks"]:
            if math.isinf(c["score"]):
                c["score"] = 1e300
    print(json.dumps(outs))


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
