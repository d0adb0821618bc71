"""GPU: the DDPM UNet (dim 64) at 96 x 96, 128 x 128 and 256 x 256, whose full-attention layers work on 144, 256 and 1024
pixels (the tiled attention kernels): loss and every parameter gradient against the CPU oracle's autograd, eps from
model_predictions, three DDIM steps, a graph-replayed training step bit-identical to eager steps, and batch consistency at
the largest batch of each size."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)      # Downsample's weight: held as [N, C, 2, 2], row-major = the reference's [N, 4 C, 1, 1]
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _hip(P, S, dev, dim=64, sampling_timesteps=None):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    net = Unet(dim=dim, channels=3)
    net.load_state_dict(P, strict=True)
    gd = GaussianDiffusion(net, img_size=S, timesteps=1000, sampling_timesteps=sampling_timesteps).to(dev)
    net.prepare_hip(dev)
    return net, gd


@pytest.mark.parametrize("S,B", [(128, 2), (96, 2), (256, 1)], ids=["128px_b2", "96px_b2", "256px_b1"])
def test_large_ddpm_step_matches_the_cpu_oracle(dev, parity, S, B):
    from oracle import diffusion as OD
    dim = 64
    P = OD.unet_init(dim=dim, channels=3, seed=S)
    g = torch.Generator().manual_seed(10 * S + B)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    loss_ref = OD.diffusion_forward(Pr, OD.diffusion_buffers(1000), img, t, noise, dim=dim)
    loss_ref.backward()
    net, gd = _hip(P, S, dev)
    loss = gd.p_losses(img.to(dev), t.to(dev), noise.to(dev), _normalize=True)
    parity("loss", abs(loss.item() - loss_ref.item()) / loss_ref.item(), RTOL)
    loss.backward()
    errs = {n: rel(p.grad, Pr[n].grad) for n, p in net.named_parameters()}
    wn = max(errs, key=errs.get)
    parity(f"worst of ALL {len(errs)} parameter gradients ({wn})", errs[wn], RTOL)


def test_eps_prediction_at_128_pixels(dev, parity):
    from oracle import diffusion as OD
    dim, S, B = 64, 128, 2
    P = OD.unet_init(dim=dim, channels=3, seed=1280)
    bufs = OD.diffusion_buffers(1000)
    g = torch.Generator().manual_seed(1281)
    x = torch.randn(B, 3, S, S, generator=g)
    t = torch.tensor([17, 803])
    with torch.no_grad():
        pn_ref, xs_ref, _ = OD.model_predictions(P, bufs, x, t, clip_x_start=False, dim=dim)
    net, gd = _hip(P, S, dev)
    pred = gd.model_predictions(x.to(dev), t.to(dev))
    parity("pred_noise (eps) 128x128", rel(pred.pred_noise, pn_ref), RTOL)
    parity("pred_x_start 128x128", rel(pred.pred_x_start, xs_ref), RTOL)


def test_three_ddim_steps_at_128_pixels(dev, parity):
    from lgm_hip import sampler
    from oracle import diffusion as OD
    dim, S, B = 64, 128, 2
    P = OD.unet_init(dim=dim, channels=3, seed=1282)
    shape = (B, 3, S, S)
    init, nz = OD.draw_loop_noise(1283, shape, 2)
    with torch.no_grad():
        ref = OD.ddim_sample_loop(P, OD.diffusion_buffers(1000), init, nz + [None], 3, dim=dim)
    net, gd = _hip(P, S, dev, sampling_timesteps=3)
    out = sampler.ddim_sample(gd, shape, init_noise=init.to(dev), noises=[n.to(dev) for n in nz] + [None])
    parity("3-pair DDIM loop at 128x128, final image", rel(out, ref), RTOL)


def _ddpm(dev, S, seed=10, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(seed)
    m = DDPM(img_channels=3, img_size=S, dim=64, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


def test_graph_replay_at_128_pixels_is_bit_identical_to_eager_steps(dev):
    """GraphedDDPMStep (the timed path) at 128 x 128, B = 8: after one replay the loss and the flat gradient buffer are
    torch.equal to an eager step fed the graph's (t, noise); after 4 replays the parameters and Adam moments are too."""
    from lgm_hip.graph import GraphedDDPMStep
    kw = dict(lr=2e-5, betas=(0.9, 0.99), ema_update_every=10, ema_decay=0.995)
    a, b = _ddpm(dev, 128, **kw), _ddpm(dev, 128, **kw)
    fa, fb = a.ema.online_model.model._flat, b.ema.online_model.model._flat
    assert torch.equal(fa.data, fb.data)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(8, 3, 128, 128, generator=g) * 2 - 1).to(dev)
    step = GraphedDDPMStep(a, oa, x.clone())
    gd_b = b.ema.online_model
    for i in range(4):
        loss_a = step.step(i).clone()
        t, noise = step.t.clone(), step.noise.clone()
        ob.zero_grad()
        loss_b = gd_b.p_losses(x, t, noise, _normalize=True)
        loss_b.backward()
        if i == 0:
            assert torch.equal(loss_a.reshape(()), loss_b.detach().reshape(())), (float(loss_a), float(loss_b))
            assert torch.equal(fa.grad, fb.grad)
            assert float(fa.grad.abs().max()) > 0
        ob.step()
        b.on_train_batch_end(None, None, i)
    assert torch.equal(fa.data, fb.data)
    sa, sb = oa._flat_state[id(fa)], ob._flat_state[id(fb)]
    assert sa["step"] == sb["step"] == 4 and torch.equal(sa["m"], sb["m"]) and torch.equal(sa["v"], sb["v"])


@pytest.mark.parametrize("S,B", [(128, 32), (256, 8)], ids=["128px_b32", "256px_b8"])
def test_batch_consistency_at_the_largest_batch(dev, parity, S, B):
    """The loss and the gradients of one batch of B equal the mean over B / 2 chunks of 2 on the same path."""
    from oracle import diffusion as OD
    P = OD.unet_init(dim=64, channels=3, seed=S + B)
    g = torch.Generator().manual_seed(S * B)
    img = torch.rand(B, 3, S, S, generator=g).to(dev)
    noise = torch.randn(B, 3, S, S, generator=g).to(dev)
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    net, gd = _hip(P, S, dev)
    flat = net._flat
    loss = gd.p_losses(img, t, noise, _normalize=True)
    loss.backward()
    full_loss, full_grad = loss.item(), flat.grad.clone()
    chunk_loss, chunk_grad = 0.0, torch.zeros_like(full_grad)
    for c in range(0, B, 2):
        flat.zero_grad()
        lc = gd.p_losses(img[c:c + 2], t[c:c + 2], noise[c:c + 2], _normalize=True)
        lc.backward()
        chunk_loss += lc.item() / (B // 2)
        chunk_grad += flat.grad / (B // 2)
    parity(f"loss, B={B} vs mean of chunks of 2", abs(full_loss - chunk_loss) / abs(chunk_loss), RTOL)
    parity(f"flat gradient, B={B} vs mean of chunks of 2", rel(full_grad, chunk_grad), RTOL)
