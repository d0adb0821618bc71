"""The ledger of the direct convolution kernels: every name the library can note from conv_igemm.hip, conv3x3.hip,
gemm_stream.hip, gemm_rows.hip and wgrad1x1.hip is RUN at the smallest shape that routes to it, `lgm_last_kernel()` is
compared for equality, and every output is compared with float64 ELEMENTWISE (oracle/bounds.py: forward error in units
of 2^-24 * S per element, tolerance measured on the float32 CPU reference by tests/test_cpu_bounds.py) as well as by the
ratio of norms the per-op tests use.  NaN-filled guard lanes around every pitched output must stay untouched.

Rows whose kernel is reachable only under an environment switch (the library reads each once per process) run in a fresh
child process per switch, one at a time; a child that ends by signal, abort or timeout fails the test and no further
child starts in the session.

The completeness tests need no GPU: every registry name is a key of LEDGER or is claimed by ELSEWHERE."""
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

RTOL = 1e-4

# name prefixes of the five direct-convolution files: a registry name that starts with one must be a key of LEDGER
DIRECT = ("igemm_kernel<", "narrow1x1_", "smalln_yx_", "wgrad_kernel<", "wgrad_group_kernel", "wgrad_reduce_batch_kernel",
          "gemm_bwd_pair_kernel", "lgm3x3::", "gemm_stream_kernel", "gemm_rows_kernel", "wgrad1x1_")

# every other name (or family prefix): the test file that runs it and asserts lgm_last_kernel
ELSEWHERE = {
    "lgmwino::wino_bwd_pair_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino::wino_wgrad_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino::wino_wgrad2_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino::wino_wgrad4_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino4::wino4_conv_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino4l::wino4l_conv_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino4w::wino4_wgrad_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino4w::wino4_wgrad2_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino4w::wino4_wgrad4_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino4w::wino4_wgrad8_kernel": "tests/test_hip_wino_ledger.py",
    "lgmwino::wino_conv_kernel": "tests/test_hip_wino_ledger.py",
    "lgmweng::weng_gemm_kernel": "tests/test_hip_weng.py",
    "linattn_bwd_fused_kernel": "tests/test_hip_attention_ledger.py",
    "linattn_out_fused_kernel": "tests/test_hip_attention_ledger.py",
    "linattn_out_kernel": "tests/test_hip_attention_ledger.py",
    "linattn_bwd_mfma": "tests/test_hip_attention_ledger.py",
    "linattn_ctx_mfma": "tests/test_hip_attention_ledger.py",
    "attn_small_fwd_kernel": "tests/test_hip_attention_ledger.py",
    "attn_small_bwd_kernel": "tests/test_hip_attention_ledger.py",
    "attn_fwd_kernel": "tests/test_hip_attention_ledger.py",
    "attn_bwd_kernel": "tests/test_hip_attention_ledger.py",
    "attn_tiled_fwd_kernel": "tests/test_hip_attention_ledger.py",
    "attn_tiled_bwd_kernel": "tests/test_hip_attention_ledger.py",
    "rms_qkv_fused_kernel": "tests/test_hip_ops.py",
    "resstack_fwd_kernel": "tests/test_hip_ops.py",
    "qsample_slice_kernel": "tests/test_hip_selfcond.py",
    "sample_step_slice_kernel": "tests/test_hip_selfcond.py",
    "selfcond_estimate_kernel": "tests/test_hip_selfcond.py",
    "cfg_mix_kernel": "tests/test_hip_classcond.py",
    "label_emb_fwd_kernel": "tests/test_hip_classcond.py",
    "label_emb_wgrad_kernel": "tests/test_hip_classcond.py",
    "gn_fused_fwd_kernel": "tests/test_hip_norm_ledger.py",
    "gn_fused_bwd_kernel": "tests/test_hip_norm_ledger.py",
    "gn_stats_kernel": "tests/test_hip_norm_ledger.py",
    "gn_bwd_reduce_kernel": "tests/test_hip_norm_ledger.py",
    "gn_coef_from_stats_kernel": "tests/test_hip_norm_ledger.py",
    "rmsnorm_fwd_kernel": "tests/test_hip_norm_ledger.py",
    "rmsnorm_bwd_kernel": "tests/test_hip_norm_ledger.py",
}

def R(name, entry, geom, why, env=None, **opts):
    return {"name": name, "entry": entry, "geom": tuple(geom), "why": why, "env": env, "opts": opts}


def _ig(mode, bm, bn, uni):
    return f"igemm_kernel<{mode}, {bm}, {bn}, {bm // 64}, {bn // 64}, {'true' if uni else 'false'}>"


# geometry = (B, H, W, Cin, Cout, k, stride, pad).  M = GEMM rows, t128 = cdiv(M, 128) * phases (dispatch_igemm), "uni" =
# launch_igemm's uniform-tap form (gathered channels % 32 == 0, strided input gradients only in residue-class form).
LEDGER = [
    # ---- implicit GEMM, forward (conv_xy) ----
    R(_ig(0, 64, 64, True), "conv_xy", (2, 16, 16, 32, 64, 4, 2, 1), "M = 128: t128 * cdiv(N, 64) = 1 < 384 -> 64x64; Cw = 32 -> uni", bias=True, res=True),
    R(_ig(0, 64, 64, True), "conv_xy", (1, 8, 8, 256, 512, 4, 2, 1), "M = 16, N = 512, K = 4096: igemm_splits = 32 planes of 4 chunks", bias=True, res=True),
    R(_ig(0, 64, 64, False), "conv_xy", (2, 16, 16, 3, 64, 4, 2, 1), "Cw = 4 is no multiple of 32 -> general decode", bias=True),
    R(_ig(0, 64, 64, False), "conv_xy", (1, 10, 6, 20, 3, 3, 1, 1), "ragged twin: M = 60 of a 64-row tile, N = 3 padded to 4, Cw = 20", bias=True, res=True),
    R(_ig(0, 128, 128, True), "conv_xy", (24, 64, 64, 32, 256, 2, 2, 0), "M = 24576: t128 = 192, cdiv(256, 128) = 2 -> 384; Cw = 32 -> uni", bias=True),
    R(_ig(0, 128, 128, True), "conv_xy", (26, 62, 62, 32, 256, 3, 2, 1), "ragged twin: M = 26 * 31 * 31 = 24986 -> t128 = 196, last tile 26 rows; padded taps", bias=True, res=True),
    R(_ig(0, 128, 128, False), "conv_xy", (24, 64, 64, 3, 256, 4, 2, 1), "M = 24576, N = 256 -> 384 tiles; Cw = 4 -> general decode", bias=True),
    R(_ig(0, 128, 128, False), "conv_xy", (26, 62, 62, 3, 256, 3, 2, 1), "ragged twin: M = 24986 -> 196 row tiles, last 26 rows; Cw = 4", bias=True, res=True),
    R(_ig(0, 128, 64, True), "conv_xy", (24, 64, 64, 32, 128, 2, 2, 0), "N = 128: t128 * cdiv(N, 128) = 192 < 384 <= t128 * cdiv(N, 64)", bias=True, res=True),
    R(_ig(0, 128, 64, True), "conv_xy", (26, 62, 62, 32, 66, 3, 2, 1), "ragged twin: M = 24986, N = 66 padded to 68 (second column tile 4 wide)", bias=True),
    R(_ig(0, 128, 64, False), "conv_xy", (24, 64, 64, 3, 128, 4, 2, 1), "as above with Cw = 4 -> general decode", bias=True),
    R(_ig(0, 128, 64, False), "conv_xy", (26, 62, 62, 3, 66, 3, 2, 1), "ragged twin: M = 24986, N = 66 padded to 68; Cw = 4", bias=True, res=True),
    # ---- implicit GEMM, input gradient (conv_yx); stride 2 with 4x4 taps and even maps runs as 4 residue classes ----
    R(_ig(1, 64, 64, True), "conv_yx", (2, 16, 16, 32, 64, 4, 2, 1), "M per class = 128, 4 classes: 4 * 1 < 384; Nw = 64 -> uni", bias=True),
    R(_ig(1, 64, 64, True), "conv_yx", (3, 12, 20, 32, 64, 4, 2, 1), "ragged twin: M per class = 3 * 6 * 10 = 180 -> 3 tiles, last 52 rows", bias=True, res=True),
    R(_ig(1, 64, 64, True), "conv_yx", (64, 1, 1, 1024, 256, 1, 1, 0), "linear: M = 64, N = 1024, K = 256, no w_t: igemm_splits = 2 planes", res=True),
    R(_ig(1, 64, 64, False), "conv_yx", (2, 16, 16, 32, 64, 3, 2, 1), "3x3 stride 2: no residue classes (KH % stride != 0) -> general decode", res=True),
    R(_ig(1, 64, 64, False), "conv_yx", (1, 10, 6, 3, 36, 3, 1, 1), "ragged twin: M = 60, N = 3 padded to 4, Nw = 36 gathered"),
    R(_ig(1, 128, 128, True), "conv_yx", (6, 64, 64, 256, 32, 4, 2, 1), "M per class = 6144: t128 = 48 * 4 = 192, cdiv(256, 128) = 2 -> 384; Nw = 32 -> uni"),
    R(_ig(1, 128, 128, True), "conv_yx", (5, 72, 72, 256, 32, 4, 2, 1), "ragged twin: M per class = 5 * 36 * 36 = 6480 -> 51 tiles, last 80 rows", res=True),
    R(_ig(1, 128, 128, False), "conv_yx", (6, 64, 64, 256, 36, 4, 2, 1), "as above with Nw = 36 gathered -> general decode", bias=True),
    R(_ig(1, 128, 128, False), "conv_yx", (5, 72, 72, 256, 36, 4, 2, 1), "ragged twin: M per class = 6480, Nw = 36", res=True),
    R(_ig(1, 128, 64, True), "conv_yx", (6, 64, 64, 128, 32, 4, 2, 1), "N = Cw = 128: 192 < 384 <= 192 * 2", res=True),
    R(_ig(1, 128, 64, True), "conv_yx", (5, 72, 72, 128, 32, 4, 2, 1), "ragged twin: M per class = 6480 -> 51 tiles, last 80 rows", bias=True),
    R(_ig(1, 128, 64, False), "conv_yx", (5, 72, 72, 128, 36, 4, 2, 1), "ragged M per class = 6480 (t128 = 204), Nw = 36 -> general decode"),
    # ---- narrow 1x1 (64 <-> 4 channels) and the image-end input gradients ----
    R("narrow1x1_fwd_kernel", "conv_xy", (7, 5, 5, 64, 3, 1, 1, 0), "narrow1x1_geom: 1x1, Cw = 64, Nw = 4; 175 pixels = 2 full trips of 64 + 47", bias=True),
    R("narrow1x1_dgrad_kernel", "conv_yx", (7, 5, 5, 64, 3, 1, 1, 0), "the same layer's input gradient (no bias, no residual)"),
    R("smalln_yx_lp_kernel<2, 2, 16>", "conv_yx", (1, 16, 32, 3, 32, 4, 2, 1), "Cw = 4, Nw = 32, class map 8 x 16: the smallest the lane-pair kernel takes (lgc = 4)", res=True),
    R("smalln_yx_lp_kernel<2, 2, 16>", "conv_yx", (2, 24, 64, 3, 64, 4, 2, 1), "class map 12 x 32: lgc = 5 (8 x 32 tiles), second row tile ragged (4 of 8 rows)", bias=True),
    R("smalln_yx_kernel<2, 2>", "conv_yx", (2, 8, 8, 3, 16, 4, 2, 1), "Nw = 16 is no multiple of 32 -> lane-group kernel, 4 lanes per pixel", res=True),
    R("smalln_yx_kernel<2, 2>", "conv_yx", (3, 64, 64, 3, 64, 4, 2, 1), "CONV_CASES image end, 16 lanes per pixel (the lane-pair kernel switched off)", env="LGM_SMALLN_LANES=1", bias=True),
    R("smalln_yx_kernel<2, 2>", "conv_yx", (2, 64, 64, 3, 128, 4, 2, 1), "CONV_CASES image end, 32 lanes per pixel", env="LGM_SMALLN_LANES=1", res=True),
    # ---- direct 3x3 (conv3x3.hip): whole 128-pixel tiles only, no ragged path ----
    R("lgm3x3::conv3x3_kernel<0>", "conv_xy", (2, 16, 16, 64, 128, 3, 1, 1), "plan_tile: 8 x 16 tiles, one image each; 2 channel phases", bias=True, res=True),
    R("lgm3x3::conv3x3_kernel<0>", "conv_xy", (4, 8, 8, 96, 64, 3, 1, 1), "8 x 8 maps: two images per tile; 3 phases of 32 channels", bias=True),
    R("lgm3x3::conv3x3_kernel<1>", "conv_yx", (2, 16, 16, 64, 128, 3, 1, 1), "input gradient from the forward weights (flipped taps)", res=True),
    R("lgm3x3::conv3x3_kernel<1>", "conv_yx", (8, 4, 4, 64, 96, 3, 1, 1), "4 x 4 maps: eight images per tile; 3 phases", bias=True),
    R("lgm3x3::conv3x3_kernel<2>", "conv_yx", (2, 16, 16, 64, 128, 3, 1, 1), "input gradient from the transposed copy w_t", wt=True, bias=True),
    R("lgm3x3::conv3x3_kernel<2>", "conv_yx", (1, 4, 64, 128, 64, 3, 1, 1), "W = 64: two 32-wide column tiles, H = 4", wt=True, res=True),
] + [
    # ---- direct 3x3 weight gradient: the fallback of the Winograd one.  TW = min(W, 32); GS by workgroups = (Nw / 64)(Cw / 64)
    #      * tile splits: <= 64 -> 4, <= 128 -> 2, else 1 (lgm_wgrad3x3_plan); total tiles = cdiv(B, images per tile) * row tiles
    R(f"lgm3x3::wgrad3x3_kernel<{tw}, {gs}>", "conv_wgrad", geom, why, env="LGM_NO_WINO=1", gbias=gb)
    for tw, gs, geom, why, gb in [
        (4, 4, (8, 4, 4, 64, 64, 3, 1, 1), "1 weight block * 1 tile of 8 images", True),
        (4, 2, (40, 4, 4, 256, 256, 3, 1, 1), "16 blocks * 5 tiles = 80 workgroups", False),
        (4, 1, (72, 4, 4, 256, 256, 3, 1, 1), "16 blocks * 9 tiles = 144 > 128", True),
        (8, 4, (2, 8, 8, 64, 64, 3, 1, 1), "1 block * 1 tile of 2 images", False),
        (8, 2, (10, 8, 8, 256, 256, 3, 1, 1), "16 blocks * 5 tiles = 80", True),
        (8, 1, (18, 8, 8, 256, 256, 3, 1, 1), "16 blocks * 9 tiles = 144", False),
        (16, 4, (1, 16, 16, 64, 128, 3, 1, 1), "2 blocks * 2 tiles", True),
        (16, 2, (3, 16, 16, 256, 256, 3, 1, 1), "16 blocks * 6 tiles = 96", False),
        (16, 1, (5, 16, 16, 256, 256, 3, 1, 1), "16 blocks * 10 tiles = 160", True),
        (32, 4, (1, 32, 32, 128, 64, 3, 1, 1), "2 blocks * 8 tiles = 16", False),
        (32, 2, (1, 32, 32, 256, 256, 3, 1, 1), "16 blocks * 8 tiles = 128", True),
        (32, 1, (2, 32, 32, 256, 256, 3, 1, 1), "16 blocks * 16 tiles = 256", False),
    ]
] + [
    # ---- generic weight gradient (conv_igemm.hip) ----
    R("wgrad_kernel<64, 64, 1, 1, true>", "conv_wgrad", (2, 16, 16, 32, 64, 4, 2, 1), "power-of-two maps -> shift/mask gather; P = 128 pixels: one split", gbias=True),
    R("wgrad_kernel<64, 64, 1, 1, true>", "conv_wgrad", (3, 64, 64, 3, 64, 4, 2, 1), "ragged twin: Q = 16 * 4 = 64 with Cw = 3 padded to 4; P = 3072 -> 12 slabs", gbias=True),
    R("wgrad_kernel<64, 64, 1, 1, false>", "conv_wgrad", (3, 12, 20, 32, 64, 4, 2, 1), "maps that are no powers of two -> general gather; P = 180 (ragged pixel chunk)", gbias=True),
    R("wgrad_kernel<64, 64, 1, 1, false>", "conv_wgrad", (1, 10, 6, 20, 36, 3, 1, 1), "ragged twin: Nw = 36 of 64 rows, Q = 180 of 192 columns, P = 60"),
    R("wgrad_kernel<128, 64, 2, 1, true>", "conv_wgrad", (1, 8, 8, 256, 1024, 4, 2, 1), "(Nw / 128) * cdiv(Q, 64) * splits = 8 * 64 * 1 >= 512", env="LGM_WGRAD_BIG=1", gbias=True),
    R("wgrad_group_kernel", "wgrad_queue", (2, 32, 32, 64, 128, 4, 2, 1), "two queued launches of the generic kernel flushed as one (P = 512: 2 slabs each)", gbias=True),
    R("wgrad_reduce_batch_kernel", "wgrad_queue", (2, 32, 32, 64, 128, 4, 2, 1), "the batched slab reducer after the queued pair", gbias=True, after="reduce"),
    R("gemm_bwd_pair_kernel", "conv_bwd_pair", (2, 8, 8, 256, 128, 1, 1, 0), "64x64 uniform input gradient (8 blocks) + generic weight gradient share one grid (<= 512 blocks)", gbias=True, res=True),
    # ---- streaming 1x1 (gemm_stream.hip): K = 32 KQ in {64, 128, 192, 256}, 64 TN columns per slice, >= 4 row tiles per
    #      workgroup: M / 64 > 3 * (256 / slices).  make_plan: TN = 2 where K <= 128 and N % 128 == 0
] + [
    R(f"gemm_stream_kernel<{kq}, {tn}, {'true' if res else 'false'}>", entry, geom, why, bias=bias, res=res, wt=(entry == "conv_yx"))
    for kq, tn, res, entry, geom, why, bias in [
        (2, 1, False, "conv_xy", (769, 8, 8, 64, 64, 1, 1, 0), "K = 64, N = 64: one slice, 769 row tiles -> 4 per workgroup, last workgroup 1", True),
        (2, 1, True, "conv_yx", (769, 8, 8, 64, 64, 1, 1, 0), "the same through conv_yx with w_t", False),
        (2, 2, False, "conv_yx", (97, 8, 8, 1024, 64, 1, 1, 0), "input gradient: N = Cw = 1024 -> 8 slices of 128, 97 row tiles -> 4 per workgroup", True),
        (2, 2, True, "conv_xy", (97, 8, 8, 64, 1024, 1, 1, 0), "K = 64, N = 1024 with residual", True),
        (4, 1, False, "conv_xy", (257, 8, 8, 128, 192, 1, 1, 0), "K = 128, N = 192 (no multiple of 128): 3 slices of 64, 257 row tiles over 85 ranges -> 4 per workgroup", False),
        (4, 1, True, "conv_xy", (769, 8, 8, 128, 64, 1, 1, 0), "K = 128, N = 64", True),
        (4, 2, False, "conv_xy", (97, 8, 8, 128, 1024, 1, 1, 0), "K = 128, N = 1024: 8 slices of 128", True),
        (4, 2, True, "conv_yx", (97, 8, 8, 1024, 128, 1, 1, 0), "input gradient with residual", False),
        (6, 1, False, "conv_xy", (97, 8, 8, 192, 512, 1, 1, 0), "K = 192: 64-column slices only; 8 slices", True),
        (6, 1, True, "conv_yx", (97, 8, 8, 512, 192, 1, 1, 0), "K = Nw = 192 gathered", True),
        (8, 1, False, "conv_yx", (97, 8, 8, 512, 256, 1, 1, 0), "K = Nw = 256 gathered", False),
        (8, 1, True, "conv_xy", (97, 8, 8, 256, 512, 1, 1, 0), "K = 256", True),
    ]
] + [
    # ---- resident-tile 1x1 (gemm_rows.hip): K % 32 == 0, K <= 256, N >= 128, M / BM >= 96 whole row tiles; BM = 128 for K <= 64
    R("gemm_rows_kernel<2>", "conv_xy", (96, 16, 8, 32, 128, 1, 1, 0), "K = 32 (not a streaming K), M = 12288 = 96 tiles of 128", bias=True, res=True),
    R("gemm_rows_kernel<2>", "conv_yx", (96, 16, 8, 192, 32, 1, 1, 0), "input gradient through w_t: K = Nw = 32, N = Cw = 192", wt=True, bias=True),
    R("gemm_rows_kernel<1>", "conv_xy", (96, 8, 8, 96, 128, 1, 1, 0), "K = 96, M = 6144 = 96 tiles of 64", bias=True),
    R("gemm_rows_kernel<1>", "conv_yx", (96, 8, 8, 128, 96, 1, 1, 0), "input gradient through w_t: K = Nw = 96", wt=True, res=True),
    # ---- streaming 1x1 weight gradient (wgrad1x1.hip): tile_of(dim) = 128 where dim % 128 == 0 else 64; splits = 256 / blocks,
    #      >= 4 chunks of 64 pixels per split: P / 64 > 3 * splits
    R("wgrad1x1_kernel<1, 1>", "conv_wgrad", (85, 8, 8, 192, 192, 1, 1, 0), "9 blocks of 64 x 64 -> 28 splits, 85 chunks -> 4 per split (last 1)", gbias=True),
    R("wgrad1x1_kernel<1, 2>", "conv_wgrad", (85, 8, 8, 384, 192, 1, 1, 0), "Nw = 192 -> 64, Cw = 384 -> 128: 9 blocks"),
    R("wgrad1x1_kernel<2, 1>", "conv_wgrad", (85, 8, 8, 192, 384, 1, 1, 0), "Nw = 384 -> 128, Cw = 192 -> 64: 9 blocks", gbias=True),
    R("wgrad1x1_kernel<2, 2>", "conv_wgrad", (85, 8, 8, 384, 384, 1, 1, 0), "9 blocks of 128 x 128"),
    R("wgrad1x1_group_kernel<1, 1>", "conv_wgrad1x1_group", (85, 8, 8, 192, 192, 1, 1, 0), "two layers (each must pass alone: 85 chunks) share the chip: 128 / 9 = 14 splits each, 7 chunks per split", gbias=True),
    R("wgrad1x1_group_kernel<1, 2>", "conv_wgrad1x1_group", (85, 8, 8, 384, 192, 1, 1, 0), "as above, 64 x 128 blocks"),
    R("wgrad1x1_group_kernel<2, 1>", "conv_wgrad1x1_group", (85, 8, 8, 192, 384, 1, 1, 0), "as above, 128 x 64 blocks", gbias=True),
    R("wgrad1x1_group_kernel<2, 2>", "conv_wgrad1x1_group", (85, 8, 8, 384, 384, 1, 1, 0), "as above, 128 x 128 blocks", gbias=True),
]

KINDS = {"conv_xy": ("xy",), "conv_yx": ("yx",), "conv_wgrad": ("wgrad",), "wgrad_queue": ("wgrad",),
         "conv_wgrad1x1_group": ("wgrad",), "conv_bwd_pair": ("yx", "wgrad")}


def row_id(row):
    return f"{row['name']}|{row['entry']}|{'x'.join(map(str, row['geom']))}"


def registry_names():
    from lgm_hip import _lib
    D = _lib.lib()._dll
    D.lgm_kernel_name.restype = ctypes.c_char_p
    return sorted({D.lgm_kernel_name(i).decode() for i in range(D.lgm_kernel_name_count())})


# ---- completeness (no GPU) ------------------------------------------------------------------------------------------------
def test_every_direct_convolution_kernel_name_has_a_ledger_row():
    names = registry_names()
    keys = {r["name"] for r in LEDGER}
    direct = [n for n in names if n.startswith(DIRECT)]
    assert len(direct) >= 50
    assert sorted(set(direct) - keys) == [], "registry names of the direct-convolution files without a ledger row"
    assert sorted(keys - set(names)) == [], "ledger rows whose name the library can never note"
    for n in names:
        if n in keys:
            continue
        assert any(n == k or n.startswith(k + "<") for k in ELSEWHERE), f"{n!r} is neither in LEDGER nor in ELSEWHERE"
    for k in ELSEWHERE:
        assert not k.startswith(DIRECT)
        assert any(n == k or n.startswith(k + "<") for n in names), f"ELSEWHERE names {k!r}, which the library never notes"
    assert len({row_id(r) for r in LEDGER}) == len(LEDGER)


def test_kernels_listed_elsewhere_are_asserted_by_the_named_test_file():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, path in ELSEWHERE.items():
        with open(os.path.join(root, path)) as fh:
            text = fh.read()
        short = name.split("::")[-1]
        assert short in text and "lgm_last_kernel" in text, f"{path} does not assert {name}"


# ---- running one row ---------------------------------------------------------------------------------------------------------
def _pad4(n):
    return (n + 3) // 4 * 4


def _guarded(dev, B, H, W, C, lo=4, hi=4):
    """A [B, H, W, C] view with pitch C + lo + hi inside a NaN-filled buffer, and the buffer."""
    buf = torch.full((B, H, W, C + lo + hi), float("nan"), device=dev)
    return buf[..., lo:lo + C], buf


def _guards_intact(buf, C, lo=4):
    return bool(torch.isnan(buf[..., :lo]).all()) and bool(torch.isnan(buf[..., lo + C:]).all())


def _nhwc(x, dev, lo=4, hi=4):
    """NCHW cpu -> channel-padded NHWC view on the GPU with pitch > C (NaN around it, zeros in the pad channels)"""
    B, C, H, W = x.shape
    view, buf = _guarded(dev, B, H, W, _pad4(C), lo, hi)
    view.zero_()
    view[..., :C] = x.permute(0, 2, 3, 1).to(dev)
    return view


def _nhwc64(t):
    """NCHW float64 -> channel-padded NHWC float64 (pad channels 0)"""
    B, C, H, W = t.shape
    out = torch.zeros(B, H, W, _pad4(C), dtype=torch.float64)
    out[..., :C] = t.permute(0, 2, 3, 1)
    return out


def _phys(w, dev=None, dtype=torch.float32):
    """OIHW -> physical [Np][T][Cp]"""
    N, C, KH, KW = w.shape
    p = torch.zeros(_pad4(N), KH * KW, _pad4(C), dtype=dtype)
    p[:N, :, :C] = w.permute(0, 2, 3, 1).reshape(N, KH * KW, C).to(dtype)
    return p if dev is None else p.to(dev)


def _vec(v, dev=None, dtype=torch.float32):
    p = torch.zeros(_pad4(v.numel()), dtype=dtype)
    p[:v.numel()] = v.reshape(-1).to(dtype)
    return p if dev is None else p.to(dev)


def _flat_guarded(dev, n, fill):
    """n floats (16-byte aligned) between two NaN guards of 32 floats"""
    buf = torch.full((n + 64,), float("nan"), device=dev)
    view = buf[32:32 + n]
    view.fill_(fill)
    return view, buf


def _flat_intact(buf, n):
    return bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[32 + n:]).all())


def _last():
    from lgm_hip import ops
    k = ops.lib()._dll.lgm_last_kernel()
    return k.decode() if k else ""


def _check(out, what, got, ref64, S64, n):
    out["checks"].append({"what": what, "score": bounds.forward_error_units(got, ref64, S64), "tol": bounds.tolerance(n),
                          "rel": bounds.rel(got, ref64)})


def _transposed(wd, geom, dev):
    from lgm_hip import ops
    Np, T, Cp = wd.shape
    wt = torch.zeros_like(wd)
    tbl = torch.tensor([[0, Np, T, Cp, 0]], dtype=torch.int32, device=dev)
    ops.lib().lgm_transpose_weights(wd.data_ptr(), wt.data_ptr(), tbl.data_ptr(), 1, ((Np + 31) // 32) * ((Cp + 31) // 32) * T,
                                    ops.stream())
    return wt


def _run_conv(row, dev, out):
    from lgm_hip import ops
    geom, o = row["geom"], row["opts"]
    B, H, W, Cin, Cout, k, s, p = geom
    yx = row["entry"] == "conv_yx"
    t = bounds.make_inputs(geom)
    Cp, Np = _pad4(Cin), _pad4(Cout)
    g = ops.make_geom(B, H, W, Cp, Np, k, k, s, p)
    wd = _phys(t["w"], dev)
    a = _nhwc(t["gy"] if yx else t["x"], dev, lo=0, hi=8)
    bias = (t["bx"] if yx else t["b"]) if o.get("bias") else None
    res = (t["res_x"] if yx else t["res_y"]) if o.get("res") else None
    oc, (oh, ow) = (Cp, (H, W)) if yx else (Np, (g.Ho, g.Wo))
    view, buf = _guarded(dev, B, oh, ow, oc)
    bd = None if bias is None else _vec(bias, dev)
    rd = None if res is None else _nhwc(res, dev, lo=4, hi=0)
    if yx:
        wt = _transposed(wd, geom, dev) if o.get("wt") else None
        ops.conv_yx(g, a, wd.data_ptr(), None if bd is None else bd.data_ptr(), rd, view, None if wt is None else wt.data_ptr())
    else:
        ops.conv_xy(g, a, wd.data_ptr(), None if bd is None else bd.data_ptr(), rd, view)
    out["name"] = _last()
    torch.cuda.synchronize()
    d = {kk: v.double() for kk, v in t.items()}
    ab = {kk: v.abs() for kk, v in d.items()}
    f = bounds.conv_yx if yx else bounds.conv_xy
    args = (lambda q: (q["gy"], q["w"], q["bx"] if bias is not None else None, q["res_x"] if res is not None else None)) if yx else \
           (lambda q: (q["x"], q["w"], q["b"] if bias is not None else None, q["res_y"] if res is not None else None))
    _check(out, "input gradient" if yx else "forward", view, _nhwc64(f(geom, *args(d))), _nhwc64(f(geom, *args(ab))),
           bounds.reduction_length("yx" if yx else "xy", geom))
    out["guards"] = _guards_intact(buf, oc)


def _wgrad_refs(geom, t, gbias):
    d = {kk: v.double() for kk, v in t.items()}
    ab = {kk: v.abs() for kk, v in d.items()}
    gw, gb = bounds.conv_wgrad(geom, d["gy"], d["x"])
    sw, sb = bounds.conv_wgrad(geom, ab["gy"], ab["x"])
    return _phys(gw, dtype=torch.float64), _phys(sw, dtype=torch.float64), _vec(gb, dtype=torch.float64), _vec(sb, dtype=torch.float64)


def _check_wgrad(out, tag, geom, gw, gb, refs, first=None):
    """gw / gb against float64; ``first`` = (gw, gb) of the run this one accumulated onto (beta = 1)"""
    rw, sw, rb, sb = refs
    n = bounds.reduction_length("wgrad", geom)
    if first is not None:
        fw, fb = first
        rw, sw = rw + fw.double().cpu().view_as(rw), sw + fw.double().cpu().view_as(sw).abs()
        if gb is not None:
            rb, sb = rb + fb.double().cpu(), sb + fb.double().cpu().abs()
    _check(out, tag + " gw", gw.view(rw.shape), rw, sw, n)
    if gb is not None:
        _check(out, tag + " gb", gb, rb, sb, n)


def _wgrad_operands(row, dev):
    from lgm_hip import ops
    geom = row["geom"]
    B, H, W, Cin, Cout, k, s, p = geom
    t = bounds.make_inputs(geom)
    Cp, Np = _pad4(Cin), _pad4(Cout)
    g = ops.make_geom(B, H, W, Cp, Np, k, k, s, p)
    return t, g, _nhwc(t["gy"], dev, lo=0, hi=4), _nhwc(t["x"], dev, lo=4, hi=4), Np * k * k * Cp, Np


def _run_wgrad(row, dev, out):
    """conv_wgrad: overwrite, name, accumulate (beta = 1), guards, and two runs give equal bits"""
    from lgm_hip import ops
    geom, gbias = row["geom"], bool(row["opts"].get("gbias"))
    t, g, gyd, xd, n_w, Np = _wgrad_operands(row, dev)
    refs = _wgrad_refs(geom, t, gbias)
    gw, wbuf = _flat_guarded(dev, n_w, 0.0)
    gb, bbuf = _flat_guarded(dev, Np, 0.0) if gbias else (None, None)
    gbp = gb.data_ptr() if gbias else None
    ops.conv_wgrad(g, gyd, xd, gw.data_ptr(), 0.0, gbp)
    out["name"] = _last()
    torch.cuda.synchronize()
    _check_wgrad(out, "overwrite", geom, gw, gb, refs)
    first = (gw.clone(), gb.clone() if gbias else None)
    ops.conv_wgrad(g, gyd, xd, gw.data_ptr(), 1.0, gbp)
    _check_wgrad(out, "beta = 1", geom, gw, gb, refs, first)
    out["guards"] = _flat_intact(wbuf, n_w) and (not gbias or _flat_intact(bbuf, Np))
    again = torch.full((n_w,), 7.0, device=dev) if (geom[3] % 4 == 0 and geom[4] % 4 == 0) else torch.zeros(n_w, device=dev)
    again_b = torch.zeros(Np, device=dev) if gbias else None
    ops.conv_wgrad(g, gyd, xd, again.data_ptr(), 0.0, again_b.data_ptr() if gbias else None)      # the same operands again
    out["deterministic"] = _last() == out["name"] and bool(torch.equal(again, first[0])) and \
        (not gbias or bool(torch.equal(again_b, first[1])))


def _run_wgrad_queue(row, dev, out):
    """two deferred, queued launches of the generic kernel -> one wgrad_group_kernel launch, then the batched reducer"""
    from lgm_hip import ops
    geom, gbias = row["geom"], bool(row["opts"].get("gbias"))
    key = (geom, gbias)
    if key in _QUEUE_RUNS:                    # one run of the scenario reports both names
        names, rec = _QUEUE_RUNS[key]
        out.update({k: v for k, v in rec.items() if k not in ("row", "name")})
        out["name"] = names[1] if row["opts"].get("after") == "reduce" else names[0]
        return
    t, g, gyd, xd, n_w, Np = _wgrad_operands(row, dev)
    refs = _wgrad_refs(geom, t, gbias)
    rows, outs = [], []
    for _ in range(2):
        gw, wbuf = _flat_guarded(dev, n_w, 0.0)
        gb, bbuf = _flat_guarded(dev, Np, 0.0)
        ops.conv_wgrad(g, gyd, xd, gw.data_ptr(), 0.0, gb.data_ptr() if gbias else None, defer=rows, queue=True)
        outs.append((gw, wbuf, gb, bbuf))
    ops.wgrad_queue_flush()
    name_flush = _last()
    assert len(rows) == 2, "the queued layers were expected to split into slabs"
    ops.wgrad_reduce_batch(rows, dev)
    name_reduce = _last()
    out["name"] = name_reduce if row["opts"].get("after") == "reduce" else name_flush
    torch.cuda.synchronize()
    for i, (gw, wbuf, gb, bbuf) in enumerate(outs):
        _check_wgrad(out, f"layer {i}", geom, gw, gb if gbias else None, refs)
    out["guards"] = all(_flat_intact(wbuf, n_w) and _flat_intact(bbuf, Np) for _, wbuf, _, bbuf in outs)
    out["deterministic"] = bool(torch.equal(outs[0][0], outs[1][0]))
    _QUEUE_RUNS[key] = ((name_flush, name_reduce), dict(out))


_QUEUE_RUNS = {}


def _run_wgrad1x1_group(row, dev, out):
    """two 1x1 layers of the row's geometry in ONE launch (overwrite, then beta = 1), through the batched slab reducer"""
    from lgm_hip import ops
    geom, gbias = row["geom"], bool(row["opts"].get("gbias"))
    t, g, gyd, xd, n_w, Np = _wgrad_operands(row, dev)
    refs = _wgrad_refs(geom, t, gbias)
    g2 = ops.make_geom(*[getattr(g, f) for f in ("B", "H", "W", "Cw", "Nw", "KH", "KW", "stride", "pad")])
    assert ops.wgrad1x1_group_supported([g, g2])
    outs = []
    for gg in (g, g2):
        gw, wbuf = _flat_guarded(dev, n_w, 3.0)
        gb, bbuf = _flat_guarded(dev, Np, -1.0)
        outs.append((gg, gw, wbuf, gb, bbuf))
    first = None
    for beta in (0.0, 1.0):
        rows = []
        ops.conv_wgrad1x1_group([(gg, gyd, xd, gw.data_ptr(), beta, gb.data_ptr() if gbias else None) for gg, gw, _, gb, _ in outs], rows)
        if beta == 0.0:
            out["name"] = _last()
        ops.wgrad_reduce_batch(rows, dev)
        torch.cuda.synchronize()
        for i, (_, gw, _, gb, _) in enumerate(outs):
            _check_wgrad(out, f"layer {i} beta = {beta:g}", geom, gw, gb if gbias else None, refs, None if first is None else first[i])
        if beta == 0.0:
            first = [(gw.clone(), gb.clone()) for _, gw, _, gb, _ in outs]
    out["guards"] = all(_flat_intact(wbuf, n_w) and _flat_intact(bbuf, Np) for _, _, wbuf, _, bbuf in outs)
    out["deterministic"] = bool(torch.equal(first[0][0], first[1][0]))


def _run_bwd_pair(row, dev, out):
    """lgm_conv_bwd_pair (ops.conv_bwd_generic): input gradient + weight gradient in one launch"""
    from lgm_hip import ops
    geom, gbias, o = row["geom"], bool(row["opts"].get("gbias")), row["opts"]
    B, H, W, Cin, Cout, k, s, p = geom
    t, g, gyd, xd, n_w, Np = _wgrad_operands(row, dev)
    refs = _wgrad_refs(geom, t, gbias)
    wd = _phys(t["w"], dev)
    Cp = _pad4(Cin)
    gx, xbuf = _guarded(dev, B, H, W, Cp)
    rd = _nhwc(t["res_x"], dev, lo=4, hi=0) if o.get("res") else None
    gw, wbuf = _flat_guarded(dev, n_w, 0.0)
    gb, bbuf = _flat_guarded(dev, Np, 0.0)
    ops.conv_bwd_generic(g, gyd, xd, wd.data_ptr(), None, gw.data_ptr(), 0.0, gb.data_ptr() if gbias else None, None, rd, gx)
    out["name"] = _last()
    torch.cuda.synchronize()
    d = {kk: v.double() for kk, v in t.items()}
    ab = {kk: v.abs() for kk, v in d.items()}
    r = lambda q: bounds.conv_yx(geom, q["gy"], q["w"], None, q["res_x"] if rd is not None else None)
    _check(out, "input gradient", gx, _nhwc64(r(d)), _nhwc64(r(ab)), bounds.reduction_length("yx", geom))
    _check_wgrad(out, "overwrite", geom, gw, gb if gbias else None, refs)
    first = (gw.clone(), gb.clone())
    ops.conv_bwd_generic(g, gyd, xd, wd.data_ptr(), None, gw.data_ptr(), 1.0, gb.data_ptr() if gbias else None, None, rd, gx)
    _check_wgrad(out, "beta = 1", geom, gw, gb if gbias else None, refs, first)
    out["guards"] = _guards_intact(xbuf, Cp) and _flat_intact(wbuf, n_w) and _flat_intact(bbuf, Np)
    gx_first = gx.clone()
    gw2, gb2 = torch.zeros(n_w, device=dev), torch.zeros(Np, device=dev)
    ops.conv_bwd_generic(g, gyd, xd, wd.data_ptr(), None, gw2.data_ptr(), 0.0, gb2.data_ptr() if gbias else None, None, rd, gx)
    out["deterministic"] = _last() == out["name"] and bool(torch.equal(gw2, first[0])) and \
        (not gbias or bool(torch.equal(gb2, first[1]))) and bool(torch.equal(gx, gx_first))


RUNNERS = {"conv_xy": _run_conv, "conv_yx": _run_conv, "conv_wgrad": _run_wgrad, "wgrad_queue": _run_wgrad_queue,
           "conv_wgrad1x1_group": _run_wgrad1x1_group, "conv_bwd_pair": _run_bwd_pair}


def run_row(row, dev):
    out = {"row": row_id(row), "name": None, "checks": [], "guards": None, "deterministic": None}
    RUNNERS[row["entry"]](row, dev, out)
    return out


def judge(row, out, parity):
    """The assertions of one row, from the record its run left (in this process or in a child)."""
    assert out["name"] == row["name"], f"{row_id(row)}: ran {out['name']!r} ({row['why']})"
    assert out["checks"]
    for c in out["checks"]:
        parity(f"{row['name']} {'x'.join(map(str, row['geom']))} {c['what']} [units of 2^-24 S]", c["score"], c["tol"])
        assert c["rel"] < RTOL, (row_id(row), c)
    assert out["guards"] is True, f"{row_id(row)}: a NaN guard lane around an output was written"
    assert out["deterministic"] in (None, True), f"{row_id(row)}: two runs of the weight gradient differ"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in LEDGER if r["env"] is None], ids=row_id)
def test_ledger_row(dev, parity, row):
    judge(row, run_row(row, dev), parity)


SWITCHES = sorted({r["env"] for r in LEDGER if r["env"]})
_CHILD_DIED = []


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
def test_switch_rows(parity, switch):
    """every row of one environment switch in a fresh child process (the library reads a switch once per process)"""
    assert not _CHILD_DIED, f"an earlier child died ({_CHILD_DIED[0]}): no further child is started in this session"
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
