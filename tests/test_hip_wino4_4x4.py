"""GPU: Winograd F(4x4,3x3) on the 4 x 4 maps (class 3 of csrc/winograd4.hip: one tile per image, 32 images per unit;
image groups of csrc/winograd4_wgrad.hip: the single tiles of four images per phase) against float64 references at the
UNet's 4 x 4 layer shapes, the weight gradient of a 4 x 4 layer sharing a grouped launch with an 8 x 8 layer, and the
selection rule (which 4 x 4 layers of the UNet take the F(4x4) kernels).  Reference op: Block.proj ddpm.py:157-173."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lightning-generative-models_amd")
F4_TOL = 2e-5        # as tests/test_hip_winograd.py: F(4x4,3x3) in fp32 is a few 1e-6 of the output scale


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def maxerr(a, ref):
    a, ref = a.double().cpu(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max())


def wino4_weights(w):
    from lgm_hip import ops
    Np, _, Cp = w.shape
    uf = torch.empty(Np * Cp * 36, device=w.device)
    ub = torch.empty(Np * Cp * 36, device=w.device)
    tab = torch.tensor([[0, Np, Cp, 0, 0, 0]], dtype=torch.int64, device=w.device)
    ops.lib().lgm_wino4_weights(w.data_ptr(), uf.data_ptr(), ub.data_ptr(), tab.data_ptr(), 1, (Np // 32) * (Cp // 32),
                                ops.stream())
    return uf, ub


def wino4(yx, g, a, u, bias, res, out, partial=False):
    from lgm_hip import ops
    L = ops.lib()
    n = L.lgm_conv3x3_wino4_workspace(ctypes.byref(g), yx)
    ws = ops.workspace(n, a.device) if n > 0 else None
    wsp, wsb = (None, 0) if ws is None else (ws.data_ptr(), ws.numel() * 4)
    if partial:
        part = (ctypes.c_int64 * 2)()
        L.lgm_conv3x3_wino4_partial(yx, ctypes.byref(g), a.data_ptr(), ops.pitch(a), u.data_ptr(),
                                    None if bias is None else bias.data_ptr(), out.data_ptr(), ops.pitch(out), wsp, wsb,
                                    ctypes.addressof(part), ops.stream())
        assert L._dll.lgm_last_kernel().decode() == "lgmwino4::wino4_conv_kernel<3, false, 0, false>"
        return ws, int(part[0]), int(part[1])
    L.lgm_conv3x3_wino4(yx, ctypes.byref(g), a.data_ptr(), ops.pitch(a), u.data_ptr(), None if bias is None else bias.data_ptr(),
                        None if res is None else res.data_ptr(), 0 if res is None else ops.pitch(res), out.data_ptr(),
                        ops.pitch(out), wsp, wsb, ops.stream())
    assert L._dll.lgm_last_kernel().decode() == "lgmwino4::wino4_conv_kernel<3, false, 0, false>"
    return n


# (B, Cin, Cout) on 4 x 4 maps: the UNet's 4 x 4 layers at the batch of 32 (one unit per 64 channels) and 128
CASES = [(32, 256, 256), (32, 512, 512), (32, 768, 512), (128, 256, 256), (128, 512, 512), (128, 768, 512), (128, 256, 512)]


@pytest.mark.parametrize("case", CASES)
def test_class3_forward_and_input_gradient(dev, case, parity):
    """Forward (+bias, +residual, split-K planes summed by the reducer or left to the consumer) and input gradient (plain
    and accumulated in place) of a 4 x 4 layer against float64; operands in channel slices of wider buffers."""
    from lgm_hip import ops
    B, ci, co = case
    H = W = 4
    gen = torch.Generator().manual_seed(B + ci + 3 * co)
    xbuf = torch.randn(B, H, W, ci + 32, generator=gen)
    ybuf = torch.randn(B, H, W, co + 64, generator=gen)
    x, y = xbuf[..., 32:], ybuf[..., :co]
    w = torch.randn(co, 9, ci, generator=gen) / (3 * ci ** 0.5)
    bias = torch.randn(co, generator=gen)
    res = torch.randn(B, H, W, co, generator=gen)
    w4 = w.reshape(co, 3, 3, ci).permute(0, 3, 1, 2).double()
    conv = F.conv2d(x.permute(0, 3, 1, 2).double(), w4, bias.double(), padding=1).permute(0, 2, 3, 1)
    ref_yx = F.conv_transpose2d(y.permute(0, 3, 1, 2).double(), w4, None, padding=1).permute(0, 2, 3, 1)
    xd, yd = xbuf.to(dev)[..., 32:], ybuf.to(dev)[..., :co]
    wd, bd, rd = w.to(dev), bias.to(dev), res.to(dev)
    uf, ub = wino4_weights(wd)
    g = ops.make_geom(B, H, W, ci, co, 3, 3, 1, 1)
    L = ops.lib()
    assert L.lgm_conv3x3_wino4_supported(ctypes.byref(g), 0) == 1 and L.lgm_conv3x3_wino4_supported(ctypes.byref(g), 1) == 1
    obuf = torch.full((B, H, W, co + 16), 7.0, device=dev)
    out = obuf[..., 16:]
    nws = wino4(0, g, xd, uf, bd, rd, out)
    parity(f"class 3 forward (+bias +residual, split-K workspace {nws} B)", maxerr(out, conv + res.double()), F4_TOL)
    assert float((obuf[..., :16] - 7.0).abs().max()) == 0           # nothing written outside the channel slice
    o2 = torch.empty(B, H, W, co, device=dev)
    wino4(0, g, xd, uf, bd, None, o2)
    parity("class 3 forward (+bias)", maxerr(o2, conv), F4_TOL)
    # partial planes (the plane-summing GroupNorm's input): their sum in plane order + bias is the reducer's result
    ws, planes, stride = wino4(0, g, xd, uf, bd, None, torch.empty_like(o2), partial=True)
    if planes > 1:
        s = ws[:stride]
        for k in range(1, planes):
            s = s + ws[k * stride:(k + 1) * stride]
        parity(f"class 3 forward from {planes} partial planes", maxerr(s.view(B, H, W, co) + bd, conv), F4_TOL)
    gx = torch.full((B, H, W, ci), float("nan"), device=dev)
    wino4(1, g, yd, ub, None, None, gx)
    parity("class 3 input gradient", maxerr(gx, ref_yx), F4_TOL)
    gx2 = torch.randn(B, H, W, ci, generator=gen).to(dev)
    ref2 = ref_yx + gx2.double().cpu()
    wino4(1, g, yd, ub, None, gx2, gx2)
    parity("class 3 input gradient accumulated in place", maxerr(gx2, ref2), F4_TOL)
    o3 = torch.empty_like(o2)
    wino4(0, g, xd, uf, bd, None, o3)
    assert torch.equal(o2, o3)                                          # fixed summation orders


@pytest.mark.parametrize("case", [(32, 256, 256), (32, 512, 512), (128, 512, 512), (128, 768, 512), (16, 256, 256)])
def test_image_group_weight_gradient(dev, case, parity):
    """lgm_conv3x3_wino4_wgrad on 4 x 4 maps (groups = the single tiles of four images): weight and fused bias gradient
    through the batched fixed-order slab reducer against float64 autograd, bit-reproducible."""
    from lgm_hip import ops
    B, ci, co = case
    H = W = 4
    gen = torch.Generator().manual_seed(B + 5 * ci + co)
    xbuf = torch.randn(B, H, W, ci + 32, generator=gen)
    ybuf = torch.randn(B, H, W, co + 64, generator=gen)
    x, y = xbuf[..., 32:], ybuf[..., :co]
    w0 = torch.zeros(co, ci, 3, 3, dtype=torch.double, requires_grad=True)
    out = F.conv2d(x.permute(0, 3, 1, 2).double(), w0, None, padding=1)
    gw_ref, = torch.autograd.grad(out, w0, y.permute(0, 3, 1, 2).double())
    gw_ref = gw_ref.permute(0, 2, 3, 1).reshape(co, 9, ci)
    gb_ref = y.double().sum((0, 1, 2))
    xd, yd = xbuf.to(dev)[..., 32:], ybuf.to(dev)[..., :co]
    g = ops.make_geom(B, H, W, ci, co, 3, 3, 1, 1)
    L = ops.lib()
    assert L.lgm_conv3x3_wino4_wgrad_supported(ctypes.byref(g)) == 1
    n = L.lgm_conv3x3_wino4_wgrad_workspace(ctypes.byref(g))
    ws = torch.empty(n // 4 + 16, device=dev)

    def run(gw, gb, beta):
        desc = (ctypes.c_int64 * 8)()
        L.lgm_conv3x3_wino4_wgrad(ctypes.byref(g), yd.data_ptr(), ops.pitch(yd), xd.data_ptr(), ops.pitch(xd), gw.data_ptr(),
                                  None if gb is None else gb.data_ptr(), beta, ws.data_ptr(), ws.numel() * 4,
                                  ctypes.addressof(desc), ops.stream())
        assert "wino4_wgrad_kernel" in L._dll.lgm_last_kernel().decode() and desc[6] >= 2
        ops.wgrad_reduce_batch([tuple(desc)], dev)
    gw = torch.full((co, 9, ci), float("nan"), device=dev)
    gb = torch.full((co,), float("nan"), device=dev)
    run(gw, gb, 0.0)
    parity("image-group F(4x4) weight gradient", maxerr(gw, gw_ref), 1e-5)
    parity("image-group F(4x4) fused bias gradient", maxerr(gb, gb_ref), 2e-6)
    gw2 = torch.ones((co, 9, ci), device=dev)
    run(gw2, None, 1.0)
    parity("image-group F(4x4) weight gradient accumulated (beta = 1)", maxerr(gw2 - 1.0, gw_ref), 1e-5)
    gw3 = torch.empty_like(gw)
    run(gw3, gb, 0.0)
    assert torch.equal(gw, gw3)


# Run in a child process: the grouped launch only takes layers the selection sends to the F(4x4) kernels, and the 4 x 4
# layers it sends there at B = 128 are too wide to share a launch.  LGM_WINO4_FORCE=1 (read once per process) sends every
# supported layer there, so a 4 x 4 layer and an 8 x 8 layer of 256 channels at B = 32 share one wino4_wgrad2 launch.
_MIXED = r"""
import ctypes, json
import torch
from lgm_hip import ops
dev = torch.device("cuda", 0)
L = ops.lib()
layers = {}
for i, (B, hw) in enumerate([(128, 4), (32, 8), (64, 4)]):
    gen = torch.Generator().manual_seed(71 + i)
    x = torch.randn(B, hw, hw, 256, generator=gen).to(dev)
    y = torch.randn(B, hw, hw, 256, generator=gen).to(dev)
    layers[(B, hw)] = (ops.make_geom(B, hw, hw, 256, 256, 3, 3, 1, 1), y, x)


def alone(l, gw, gb):
    g = l[0]
    ws = torch.empty(L.lgm_conv3x3_wino4_wgrad_workspace(ctypes.byref(g)) // 4 + 16, device=dev)
    desc = (ctypes.c_int64 * 8)()
    L.lgm_conv3x3_wino4_wgrad(ctypes.byref(g), l[1].data_ptr(), ops.pitch(l[1]), l[2].data_ptr(), ops.pitch(l[2]),
                              gw.data_ptr(), gb.data_ptr(), 0.0, ws.data_ptr(), ws.numel() * 4, ctypes.addressof(desc),
                              ops.stream())
    ops.wgrad_reduce_batch([tuple(desc)], dev)
    return int(desc[6])


res = {}
# the same MFMA work on both layers: the chip's 256 workgroups are shared 128 / 128, which a stand-alone launch reproduces
# under a CU margin of 128 (same budget -> same slab count -> the same summation order)
for name, pick in (("4x4+8x8", [(128, 4), (32, 8)]), ("8x8+4x4+4x4", [(32, 8), (128, 4), (64, 4)])):
    ls = [layers[k] for k in pick]
    res[name + " supported"] = bool(ops.wgrad_group_supported([l[0] for l in ls]))
    gws = [torch.full((256, 9, 256), float("nan"), device=dev) for _ in ls]
    gbs = [torch.full((256,), float("nan"), device=dev) for _ in ls]
    rows = []
    ops.conv_wgrad_group([(l[0], l[1], l[2], gw.data_ptr(), 0.0, gb.data_ptr()) for l, gw, gb in zip(ls, gws, gbs)], rows)
    res[name + " kernel"] = L._dll.lgm_last_kernel().decode()
    res[name + " splits"] = [int(r[6]) for r in rows]          # (before the reduction: it empties the list)
    ops.wgrad_reduce_batch(rows, dev)
    for l, gw in zip(ls, gws):
        w0 = torch.zeros(256, 256, 3, 3, dtype=torch.double, requires_grad=True)
        out = torch.nn.functional.conv2d(l[2].cpu().permute(0, 3, 1, 2).double(), w0, None, padding=1)
        gref, = torch.autograd.grad(out, w0, l[1].cpu().permute(0, 3, 1, 2).double())
        gref = gref.permute(0, 2, 3, 1).reshape(256, 9, 256)
        res.setdefault(name + " errors", []).append(float((gw.double().cpu() - gref).abs().max() / gref.abs().max()))
    if len(ls) == 2:
        L.lgm_set_cu_margin(128)
        try:
            same, splits = True, []
            for l, gw, gb in zip(ls, gws, gbs):
                aw, ab = torch.empty_like(gw), torch.empty_like(gb)
                splits.append(alone(l, aw, ab))
                same = same and torch.equal(aw, gw) and torch.equal(ab, gb)
        finally:
            L.lgm_set_cu_margin(-1)
        res[name + " alone splits"] = splits
        res[name + " equal"] = same
print("RESULT " + json.dumps(res))
"""


def test_weight_gradients_of_4x4_and_8x8_layers_share_one_launch(parity):
    """A 4 x 4 layer's F(4x4) weight gradient (image groups) shares the grouped launch with an 8 x 8 layer's (2 x 2-tile
    groups): wino4_wgrad2 / wino4_wgrad4 kernels, each layer against float64, and the pair torch.equal to the layers'
    own launches planned on the same share of the chip."""
    env = dict(os.environ, LGM_WINO4_FORCE="1", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _MIXED], env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    for name, kern in (("4x4+8x8", "wino4_wgrad2_kernel"), ("8x8+4x4+4x4", "wino4_wgrad4_kernel")):
        assert res[name + " supported"], res
        assert kern in res[name + " kernel"], res
        for k, e in enumerate(res[name + " errors"]):
            parity(f"{name}: layer {k} of the grouped F(4x4) weight gradient", e, 1e-5)
    assert res["4x4+8x8 alone splits"] == res["4x4+8x8 splits"], res
    assert res["4x4+8x8 equal"], res


def test_selection_of_the_unet_4x4_layers():
    """Which kernel family each 3x3 layer of the UNet's 4 x 4 level gets: F(4x4) (class 3) for the 512- and 768-channel
    layers at B = 128, the F(2x2) pair for the 256-channel layers and at small batches."""
    from lgm_hip import ops
    L = ops.lib()

    def pref(B, ci, co, yx):
        g = ops.make_geom(B, 4, 4, ci, co, 3, 3, 1, 1)
        return int(L.lgm_conv3x3_wino4_preferred(ctypes.byref(g), yx))
    for yx in (0, 1):
        assert pref(128, 512, 512, yx) == 1
        assert pref(128, 768, 512, yx) == 1
        assert pref(128, 256, 256, yx) == 0
        assert pref(128, 256, 512, yx) == 0
        assert pref(128, 512, 256, yx) == 0
        for B in (16, 32, 64):
            for ci, co in ((512, 512), (768, 512), (256, 256)):
                assert pref(B, ci, co, yx) == 0, (B, ci, co, yx)
    g = ops.make_geom(128, 4, 4, 512, 512, 3, 3, 1, 1)
    assert L.lgm_conv3x3_wino4_wgrad_supported(ctypes.byref(g)) == 1
    # light workgroups asked for (a collective beside the launches): the F(2x2) pair keeps the 4 x 4 layers
    L.lgm_wino4_set_light(1)
    try:
        assert pref(128, 512, 512, 0) == 0 and pref(128, 512, 512, 1) == 0
    finally:
        L.lgm_wino4_set_light(-1)
    assert pref(128, 512, 512, 0) == 1
