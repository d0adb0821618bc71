"""Generate tests/golden/pixelcnn.npz: the REAL reference's ``PixelCNN(8, 16, 12, num_layers=2)`` on a 5 x 6 grid, B = 3, on the
CPU in float32 and float64: logits, ``CrossEntropyLoss`` and every gradient, plus a 12 x 8 codebook and one sampled chain.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_edm.py, whose stubs (oracle.make_golden.install_stubs) and ``--check`` mode it
shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_pixelcnn.py [--check]

Recipe: weights ``tests/pixelcnn_ref.init(8, 16, 12, 2, seed=2201)`` (normal, dead taps zero; recorded AFTER masking: the
reference's first forward multiplies by the mask, which changes nothing), data seed 2202.  Stored: the reference's state-dict
keys, shapes and parameter order; the input, the targets, the logits in float32 and float64, the loss in both, every
gradient (whole up to 512 elements, else the norm over its live taps + a 256-element strided sample of them); the codebook,
the chain's uniforms and its codes.
The chain: per position a whole float64 forward of the reference; the tool picks a class with float64 probability > 1e-3 and
sets u = cdf[c - 1] + f p_c with f in [0.1, 0.9], so u sits >= 1e-4 from every boundary of the float64 CDF.  It asserts that
margin on the stored float32 u, and that a float32 CPU chain (sequential float32 CDF) draws the same codes."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "pixelcnn.npz")

CIN, HID, K, LAYERS, H, W, B = 8, 16, 12, 2, 5, 6, 3
SEED, DATA_SEED, CHAIN_SEED = 2201, 2202, 2203
WHOLE, SAMPLE = 512, 256
MARGIN, P_MIN = 1e-4, 1e-3


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.autoregressive import pixelcnn as R
    import pixelcnn_ref as PR

    torch.set_num_threads(8)
    P = PR.init(CIN, HID, K, LAYERS, SEED)
    g = torch.Generator().manual_seed(DATA_SEED)
    x = torch.randn(B, CIN, H, W, generator=g)
    target = torch.randint(0, K, (B, H, W), generator=g)
    codebook = torch.randn(K, CIN, generator=g)

    def network(double=False):
        net = R.PixelCNN(CIN, HID, K, num_layers=LAYERS)
        net.load_state_dict(P, strict=True)
        return net.double() if double else net

    net = network()
    fx = {"cin": CIN, "hid": HID, "K": K, "layers": LAYERS, "H": H, "W": W, "B": B, "seed": SEED, "grad_sample": SAMPLE,
          "keys": np.asarray(list(net.state_dict().keys())),
          "shapes": np.asarray([",".join(map(str, v.shape)) for v in net.state_dict().values()]),
          "param_order": np.asarray([n for n, _ in net.named_parameters()]),
          "x": x.numpy(), "target": target.numpy(), "codebook": codebook.numpy()}
    for k, v in net.state_dict().items():
        if k.endswith(".mask"):
            assert torch.equal(v, P[k]), k

    logits = net(x)
    loss = torch.nn.CrossEntropyLoss()(logits, target)
    loss.backward()
    for k, v in net.state_dict().items():                    # the forward's ``weight.data *= mask`` changed nothing
        assert torch.equal(v, P[k]), k
    n64 = network(True)
    with torch.no_grad():
        logits64 = n64(x.double())
        loss64 = torch.nn.CrossEntropyLoss()(logits64, target)
    P64 = {k: v.double() for k, v in P.items()}
    assert float((PR.forward(P64, x.double()) - logits64).abs().max()) < 1e-12      # the restatement is the reference
    fx["logits"], fx["logits64"] = logits.detach().numpy(), logits64.numpy()
    fx["loss"], fx["loss64"] = loss.detach().numpy(), loss64.numpy()
    for n, p in net.named_parameters():
        grad = p.grad
        if n.endswith(".weight") and n.replace(".weight", ".mask") in P:
            live = P[n.replace(".weight", ".mask")] > 0
            flat = grad[live]                                # the live taps, in the tensor's row-major order
        else:
            flat = grad.reshape(-1)
        if flat.numel() <= WHOLE:
            fx[f"grad:{n}"] = flat.numpy().copy()
        else:
            fx[f"gradnorm:{n}"] = np.float64(flat.double().norm().item())
            fx[f"gradsample:{n}"] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
    print(f"loss {float(loss.detach()):.6f} (float64 {float(loss64):.6f})")

    # the chain
    gc = torch.Generator().manual_seed(CHAIN_SEED)
    xin = torch.zeros(B, CIN, H, W, dtype=torch.float64)
    codes = torch.zeros(B, H, W, dtype=torch.int64)
    uniforms = torch.zeros(H * W, B, dtype=torch.float32)
    with torch.no_grad():
        for p in range(H * W):
            i, j = divmod(p, W)
            prob = torch.softmax(n64(xin)[:, :, i, j], dim=-1)
            cdf = torch.cumsum(prob, dim=-1)
            for b in range(B):
                ok = torch.nonzero(prob[b] > P_MIN).reshape(-1)
                c = int(ok[int(torch.randint(0, ok.numel(), (1,), generator=gc))])
                f = 0.1 + 0.8 * float(torch.rand(1, generator=gc))
                u = np.float32(float(cdf[b, c - 1] if c > 0 else 0.0) + f * float(prob[b, c]))
                assert float((cdf[b] - float(u)).abs().min()) >= MARGIN and MARGIN <= float(u) < 1.0, (p, b, float(u))
                uniforms[p, b] = float(u)
                codes[b, i, j] = c
            xin[:, :, i, j] = codebook[codes[:, i, j]].double()
    codes32, _ = PR.chain(P, codebook, uniforms, H, W)
    assert torch.equal(codes32, codes), "the float32 chain draws other codes"
    codes64, _ = PR.chain(P64, codebook.double(), uniforms, H, W)
    assert torch.equal(codes64, codes)
    fx["uniforms"], fx["codes"] = uniforms.numpy(), codes.numpy()
    print(f"chain: {len(set(codes.reshape(-1).tolist()))} distinct classes drawn over {B * H * W} positions")
    return {k: np.asarray(v) for k, v in fx.items()}


if __name__ == "__main__":
    fx = generate()
    if "--check" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as d:
            np.savez_compressed(os.path.join(d, "again.npz"), **fx)
            same = open(os.path.join(d, "again.npz"), "rb").read() == open(OUT, "rb").read()
        print(f"{OUT}: {'identical' if same else 'DIFFERS'}")
        sys.exit(0 if same else 1)
    np.savez_compressed(OUT, **fx)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
