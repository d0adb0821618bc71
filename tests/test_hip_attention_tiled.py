"""GPU: the tiled full-attention kernels (csrc/attention_tiled.hip) that lgm_attn_fwd / lgm_attn_bwd run for more than 128
query pixels, against a float64 CPU restatement of the attention core (ddpm.py Attention: softmax(q k^T * scale) v with
M memory rows in front of the keys): out, lse, the qkv gradient and the memory rows' gradient at 1e-4 relative, with
strided operands, gmem_beta = 1, the deferred reducer and reproducibility; LGM_TILED_ATTN=1 at the small shapes."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lightning-generative-models_amd")


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


def reference(qkv, mem, gout, heads):
    """float64: out [B, hidden, H, W], lse [B, heads, n], d qkv, d mem for the upstream gradient gout."""
    B, _, H, W = qkv.shape
    d, n = 32, H * W
    qkv = qkv.double().requires_grad_(True)
    mem = mem.double().requires_grad_(True)
    q, k, v = (t.reshape(B, heads, d, n).transpose(-1, -2) for t in qkv.chunk(3, dim=1))
    mk, mv = (m.unsqueeze(0).expand(B, -1, -1, -1) for m in mem)
    k = torch.cat((mk, k), dim=-2)
    v = torch.cat((mv, v), dim=-2)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * d ** -0.5
    lse = s.logsumexp(dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", s.softmax(dim=-1), v).transpose(-1, -2).reshape(B, heads * d, H, W)
    out.backward(gout.double())
    return out.detach(), lse.detach(), qkv.grad, mem.grad


def strided(x, dev, offset, extra):
    """NCHW cpu -> NHWC cuda view [..., offset:offset + C] of a NaN-filled wider buffer (row pitch C + extra)."""
    B, C, H, W = x.shape
    buf = torch.full((B, H, W, C + extra), float("nan"), device=dev)
    view = buf[..., offset:offset + C]
    view.copy_(x.permute(0, 2, 3, 1))
    return view


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def run_case(dev, B, heads, H, W, M, seed):
    """HIP forward + backward (direct path, gmem_beta = 0) on strided operands; returns the inputs, reference and results."""
    from lgm_hip import ops
    d, hidden = 32, heads * 32
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * hidden, H, W, generator=g)
    mem = torch.randn(2, heads, M, d, generator=g)
    gout = torch.randn(B, hidden, H, W, generator=g)
    qd = strided(qkv, dev, 1, 7)                          # a channel slice: unaligned base, odd pitch
    god = strided(gout, dev, 3, 5)
    memd = torch.zeros(max(mem.numel(), 4) + 4, device=dev)
    memd[:mem.numel()] = mem.reshape(-1).to(dev)
    od = strided(torch.zeros(B, hidden, H, W), dev, 2, 6)
    lse = ops.attn_fwd(qd, memd.data_ptr(), heads, d, M, od)
    gq = strided(torch.zeros(B, 3 * hidden, H, W), dev, 0, 9)
    gm = torch.zeros(max(mem.numel(), 4), device=dev)
    ops.attn_bwd(qd, memd.data_ptr(), od, god, lse, heads, d, M, gq, gm.data_ptr(), 0.0)
    return dict(qkv=qkv, mem=mem, gout=gout, qd=qd, god=god, memd=memd, od=od, lse=lse, gq=gq, gm=gm,
                ref=reference(qkv, mem, gout, heads))


SHAPES = [(2, 4, 12, 12), (2, 2, 9, 15), (2, 4, 16, 16), (1, 4, 32, 32), (1, 1, 40, 40)]
CASES = [(s, M) for s in SHAPES for M in (0, 4)] + [(SHAPES[0], 16)]


@pytest.mark.parametrize("shape,M", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}-M{M}" for s, M in CASES])
def test_tiled_attention_matches_float64(dev, parity, shape, M):
    B, heads, H, W = shape
    assert H * W > 128                                    # the tiled kernels without any switch
    r = run_case(dev, B, heads, H, W, M, seed=H * W + M)
    out_ref, lse_ref, gqkv_ref, gmem_ref = r["ref"]
    parity("out", rel(nchw(r["od"]), out_ref), RTOL)
    parity("lse", rel(r["lse"], lse_ref), RTOL)
    parity("qkv gradient", rel(nchw(r["gq"]), gqkv_ref), RTOL)
    assert not torch.isnan(r["gq"]).any() and not torch.isnan(r["od"]).any()
    if M:
        parity("memory rows gradient", rel(r["gm"][:r["mem"].numel()], gmem_ref.reshape(-1)), RTOL)


@pytest.mark.parametrize("shape,M", [((2, 4, 12, 12), 4), ((2, 2, 9, 15), 16), ((1, 4, 32, 32), 4)])
def test_tiled_backward_beta_deferred_and_reproducible(dev, shape, M):
    """gmem_beta = 1 adds to what is there; the deferred reducer gives the direct path's bits; two runs give equal bits."""
    from lgm_hip import ops
    B, heads, H, W = shape
    r = run_case(dev, B, heads, H, W, M, seed=7 * H * W + M)
    nm = r["mem"].numel()
    args = (r["qd"], r["memd"].data_ptr(), r["od"], r["god"], r["lse"], heads, 32, M)
    gq2 = torch.zeros_like(r["gq"])
    gm2 = torch.zeros_like(r["gm"])
    ops.attn_bwd(*args, gq2, gm2.data_ptr(), 0.0)
    assert torch.equal(gq2, r["gq"]) and torch.equal(gm2, r["gm"])
    base = torch.linspace(-1, 1, r["gm"].numel(), device=dev)
    gm_b = base.clone()
    ops.attn_bwd(*args, torch.zeros_like(r["gq"]), gm_b.data_ptr(), 1.0)
    assert rel(gm_b[:nm] - base[:nm], r["ref"][3].reshape(-1)) < RTOL
    gm_d, gq_d, rows = base.clone(), torch.zeros_like(r["gq"]), []
    ops.attn_bwd(*args, gq_d, gm_d.data_ptr(), 1.0, defer=rows)
    assert len(rows) == 1
    ops.wgrad_reduce_batch(rows, dev)
    assert torch.equal(gq_d, r["gq"])
    assert torch.equal(gm_d, gm_b)


_CHILD = r"""
import json, sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
sys.path.insert(0, sys.argv[3])
import test_hip_attention_tiled as T
dev = torch.device("cuda", 0)
errs = {}
for B, heads, H, W in ((2, 4, 4, 4), (2, 2, 3, 5), (1, 4, 8, 16)):
    for M in (0, 4):
        r = T.run_case(dev, B, heads, H, W, M, seed=H * W + M)
        out_ref, lse_ref, gqkv_ref, gmem_ref = r["ref"]
        e = [T.rel(T.nchw(r["od"]), out_ref), T.rel(r["lse"], lse_ref), T.rel(T.nchw(r["gq"]), gqkv_ref)]
        if M:
            e.append(T.rel(r["gm"][:r["mem"].numel()], gmem_ref.reshape(-1)))
        errs[f"{B}x{heads}x{H}x{W}-M{M}"] = max(e)
print("ERRS " + json.dumps(errs))
"""


def test_forced_tiled_kernels_at_small_shapes(parity):
    """LGM_TILED_ATTN=1 (read once per process, hence a fresh child) runs the tiled kernels at n <= 128."""
    env = dict(os.environ, LGM_TILED_ATTN="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, PKG, os.path.join(ROOT, "tests")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ERRS ")][-1]
    errs = json.loads(line[5:])
    assert len(errs) == 6
    for k, e in errs.items():
        parity(f"LGM_TILED_ATTN=1 {k}", e, RTOL)


def test_attend_module_at_256_pixels(dev, parity):
    """models.modules.attend.Attend at n = 256 (no longer refused): forward and autograd backward against torch."""
    from models.modules.attend import Attend
    g = torch.Generator().manual_seed(256)
    q, k, v = (torch.randn(2, 4, 256, 32, generator=g) for _ in range(3))
    go = torch.randn(2, 4, 256, 32, generator=g)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = torch.softmax(qr @ kr.transpose(-1, -2) * 32 ** -0.5, dim=-1) @ vr
    ref.backward(go.double())
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = Attend()(qd, kd, vd)
    parity("Attend n=256 out", rel(out, ref), RTOL)
    out.backward(go.to(dev))
    for name, a, b in (("q", qd, qr), ("k", kd, kr), ("v", vd, vr)):
        parity(f"Attend n=256 d{name}", rel(a.grad, b.grad), RTOL)
