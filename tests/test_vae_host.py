"""The MLP VAE without a GPU: the library's new symbols and their argument checks, the module's surface against the
reference's (keys and parameter order written out), the CPU path against a plain torch restatement to the bit,
tests/vae_ref.py against float64 autograd, the fixture's margins, and the float32 CPU score of every shape that
tests/test_hip_vae.py runs on the device (so the bound there is set by the reference's own float32, not by the kernels)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

import vae_ref as VR
from oracle import bounds

ENTRY_POINTS = ("lgm_dense_fwd_workspace", "lgm_dense_fwd", "lgm_dense_bwd_workspace", "lgm_dense_bwd", "lgm_vae_head_fwd",
                "lgm_vae_head_bwd_workspace", "lgm_vae_head_bwd", "lgm_tanh_l1_fwd", "lgm_tanh_l1_bwd", "lgm_vae_loss")

# reference models/generative/vae/vae.py:40-51, :76-85 - written out, not derived
REF_KEYS = ["encoder.layers.0.weight", "encoder.layers.0.bias", "encoder.layers.2.weight", "encoder.layers.2.bias",
            "encoder.layers.4.weight", "encoder.layers.4.bias", "encoder.mu.weight", "encoder.mu.bias",
            "encoder.log_var.weight", "encoder.log_var.bias", "decoder.layers.0.weight", "decoder.layers.0.bias",
            "decoder.layers.2.weight", "decoder.layers.2.bias", "decoder.layers.4.weight", "decoder.layers.4.bias",
            "decoder.layers.6.weight", "decoder.layers.6.bias"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "vae.npz")))


def _lib():
    from lgm_hip import _lib
    return _lib.lib()


def test_header_prototypes_and_exported_symbols():
    from lgm_hip import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in protos, f"{name} is not declared in include/lgm_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert _lib.ABI_VERSION == 8


def test_entry_points_reject_bad_arguments_before_any_launch():
    from lgm_hip._lib import LgmArgumentError
    L = _lib()
    P = 4096                     # a non-null, 16-byte aligned address that is never dereferenced: every call is refused first
    ok_fwd = dict(x=P, xp=8, w=P, b=P, B=2, K=8, N=8, act=0, slope=0.0, y=P, yp=8, ws=None, wsb=0)

    def fwd(**kw):
        a = dict(ok_fwd, **kw)
        L.lgm_dense_fwd(a["x"], a["xp"], a["w"], a["b"], a["B"], a["K"], a["N"], a["act"], a["slope"], a["y"], a["yp"], a["ws"],
                        a["wsb"], None)
    for bad in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(K=0), dict(N=0), dict(xp=7), dict(yp=7), dict(act=1),
                dict(act=3), dict(act=6), dict(w=P + 4)):
        with pytest.raises(LgmArgumentError):
            fwd(**bad)
    with pytest.raises(LgmArgumentError):                 # a split plan without its workspace
        L.lgm_dense_fwd(P, 784, P, P, 32, 784, 512, 0, 0.0, P, 512, None, 0, None)
    assert L.lgm_dense_fwd_workspace(32, 784, 512) > 0 and L.lgm_dense_fwd_workspace(512, 256, 512) == 0
    assert L.lgm_dense_fwd_workspace(0, 8, 8) < 0 and L.lgm_dense_bwd_workspace(2, 0, 8, 1) < 0
    assert L.lgm_vae_head_bwd_workspace(0, 4) < 0 and L.lgm_vae_head_bwd_workspace(3, 3) == 2 * 3 * 4 * 4
    nb = L.lgm_dense_bwd_workspace(2, 8, 8, 1)
    assert nb >= 2 * 8 * 4

    def bwd(gy=P, gyp=8, y=P, yp=8, x=P, xp=8, wt=P, B=2, K=8, N=8, act=4, gx=P, gxp=8, gw=P, gb=P, ws=P, wsb=None):
        L.lgm_dense_bwd(gy, gyp, y, yp, x, xp, wt, B, K, N, act, 0.2, gx, gxp, gw, gb, 1.0, ws, nb if wsb is None else wsb, None)
    for bad in (dict(gy=None), dict(x=None), dict(gw=None), dict(ws=None), dict(B=0), dict(gyp=7), dict(xp=7), dict(yp=7),
                dict(gxp=7), dict(act=2), dict(y=None), dict(wt=None), dict(wsb=nb - 4)):
        with pytest.raises(LgmArgumentError):
            bwd(**bad)
    # heads
    with pytest.raises(LgmArgumentError):
        L.lgm_vae_head_fwd(None, 128, P, P, P, P, P, 2, 128, 4, P, P, P, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_vae_head_fwd(P, 127, P, P, P, P, P, 2, 128, 4, P, P, P, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_vae_head_fwd(P, 128, P, P, P, P, P, 0, 128, 4, P, P, P, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_vae_head_bwd(P, P, P, P, P, 0.01, P, 128, P, P, 2, 128, 4, P, 128, P, P, P, P, 0.0, None, 0, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_vae_head_bwd(P, P, P, P, P, 0.01, P, 128, P, P, 2, 128, 4, P, 127, P, P, P, P, 0.0, P, 1 << 20, None)
    # loss
    with pytest.raises(LgmArgumentError):
        L.lgm_tanh_l1_fwd(P, 64, None, 64, 2, 64, P, 64, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_tanh_l1_fwd(P, 63, P, 64, 2, 64, P, 64, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_tanh_l1_bwd(P, 64, P, 64, None, 2, 64, P, 64, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_tanh_l1_bwd(P, 64, P, 64, P, 0, 64, P, 64, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_vae_loss(P, None, 2, 64, 4, 0.01, P, None)


def test_split_plan_does_not_depend_on_the_cu_margin():
    L = _lib()
    try:
        sizes = []
        for margin in (0, 16):
            L.lgm_set_cu_margin(margin)
            sizes.append([L.lgm_dense_fwd_workspace(B, K, N) for B, K, N in VR.DENSE_SHAPES]
                         + [L.lgm_dense_bwd_workspace(B, K, N, 1) for B, K, N in VR.DENSE_SHAPES])
    finally:
        L.lgm_set_cu_margin(-1)
    assert sizes[0] == sizes[1]


def _vae(**kw):
    from models.generative.vae.vae import VAE
    return VAE(**kw)


def test_module_surface_keys_and_parameter_order():
    from models.generative.vae.vae import Decoder
    m = _vae(img_channels=1, img_size=8, latent_dim=4)
    for name in ("make_fast_step", "encode", "decode", "reconstruct", "sample", "prepare_hip"):
        assert callable(getattr(m, name)), name
    assert callable(Decoder.random_sample)
    assert list(m.state_dict().keys()) == REF_KEYS == VR.KEYS
    assert [n for n, _ in m.named_parameters()] == REF_KEYS
    sizes = VR.layer_sizes(1, 8, 4)
    for k, v in m.state_dict().items():
        fin, fout = sizes[k.rsplit(".", 1)[0]]
        assert tuple(v.shape) == ((fout, fin) if k.endswith("weight") else (fout,)), k
    assert m.prepare_hip("cpu") is None and m._flat is None          # a no-op on the CPU
    assert all(type(p) is nn.Parameter and not hasattr(p, "_lgm_flat") for p in m.parameters())
    assert type(m.configure_optimizers()) is torch.optim.Adam
    assert tuple(m.decoder.random_sample(3).shape) == (3, 1, 8, 8)
    assert "not on the HIP hot path" not in __import__("models.generative.vae.vae", fromlist=["x"]).__doc__


def test_sample_and_decode_refuse_a_wrong_z():
    m = _vae(img_channels=1, img_size=8, latent_dim=4)
    for z in (torch.zeros(3, 5), torch.zeros(4), torch.zeros(3, 4, 1)):
        with pytest.raises(ValueError):
            m.decode(z)
        with pytest.raises(ValueError):
            m.sample(3, z=z)
    with pytest.raises(ValueError):
        m.sample(2, z=torch.zeros(3, 4))
    z = torch.randn(3, 4)
    assert torch.equal(m.sample(3, z=z), m.decode(z)) and torch.equal(m.decode(z), m.decoder(z).detach())
    x = torch.rand(2, 1, 8, 8) * 2 - 1
    mu, lv = m.encode(x)
    assert torch.equal(mu, m.encoder(x)[0].detach()) and torch.equal(m.reconstruct(x), m.decode(mu))
    assert tuple(m.sample(5).shape) == (5, 1, 8, 8)


def _plain_torch_vae(C, S, L):
    """The model as the parent commit built it: nn.Linear / nn.Sequential, in the same construction order"""
    D = C * S * S
    enc = nn.Sequential(nn.Linear(D, 512), nn.LeakyReLU(0.2), nn.Linear(512, 256), nn.LeakyReLU(0.2), nn.Linear(256, 128),
                        nn.LeakyReLU(0.2))
    mu, lv = nn.Linear(128, L), nn.Linear(128, L)
    dec = nn.Sequential(nn.Linear(L, 128), nn.LeakyReLU(0.2), nn.Linear(128, 256), nn.LeakyReLU(0.2), nn.Linear(256, 512),
                        nn.LeakyReLU(0.2), nn.Linear(512, D), nn.Tanh())
    return enc, mu, lv, dec


def test_cpu_path_is_bit_equal_to_a_plain_torch_restatement():
    C, S, L, B, kw = 1, 8, 4, 4, 1e-2
    torch.manual_seed(11)
    m = _vae(img_channels=C, img_size=S, latent_dim=L, kld_weight=kw)
    after_m = torch.rand(1)
    torch.manual_seed(11)
    enc, mu_l, lv_l, dec = _plain_torch_vae(C, S, L)
    assert torch.equal(torch.rand(1), after_m), "the constructor draws what nn.Linear draws, no more"
    plain = [p for mod in (enc, mu_l, lv_l, dec) for p in mod.parameters()]
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), plain))
    x = torch.rand(B, C, S, S, generator=torch.Generator().manual_seed(3)) * 2 - 1
    torch.manual_seed(5)
    loss = m.training_step((x, None), 0)
    loss.backward()
    torch.manual_seed(5)
    h = enc(x.flatten(1))
    mu, lv = mu_l(h), lv_l(h)
    xh = dec(mu + torch.randn_like(mu) * torch.exp(lv / 2)).view(-1, C, S, S)
    recon = torch.nn.functional.l1_loss(xh, x)
    kld = -0.5 * torch.mean(1 + lv - mu.pow(2) - lv.exp())
    ref = recon + kw * kld
    ref.backward()
    assert torch.equal(loss, ref) and torch.equal(m.logged["train_recon_loss"], recon) and torch.equal(m.logged["train_kld"], kld)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(m.parameters(), plain))


@pytest.mark.parametrize("dims", [(1, 8, 4, 4), (3, 5, 3, 3)])
def test_vae_ref_against_float64_autograd(dims):
    C, S, L, B = dims
    P = {k: v.double() for k, v in VR.vae_init(C, S, L, 7).items()}
    m = _vae(img_channels=C, img_size=S, latent_dim=L, kld_weight=0.3).double()
    m.load_state_dict(P)
    g = torch.Generator().manual_seed(8)
    x, eps = torch.rand(B, C, S, S, generator=g).double() * 2 - 1, torch.randn(B, L, generator=g).double()
    mu, lv = m.encoder(x)
    xh = m.decoder(mu + eps * torch.exp(lv / 2))
    loss = torch.nn.functional.l1_loss(xh, x) + 0.3 * (-0.5 * torch.mean(1 + lv - mu.pow(2) - lv.exp()))
    (2.5 * loss).backward()
    o, tape = VR.forward(P, x, eps, 0.3)
    G = VR.backward(P, tape, 0.3, gloss=2.5)
    assert abs(float(o["loss"] - loss.detach())) < 1e-12
    assert float((o["x_hat"].view_as(xh) - xh.detach()).abs().max()) < 1e-12
    for n, p in m.named_parameters():
        assert float((G[n] - p.grad).abs().max()) < 1e-12, n


def test_fixture_holds_its_margins_and_agrees_with_vae_ref(fx):
    assert fx["cases"].tolist() == ["a", "b"]
    assert [fx[f"{c}:dims"].tolist() for c in ("a", "b")] == [[1, 8, 4, 4], [3, 5, 3, 3]]
    kw = float(fx["kld_weight"])
    for c in ("a", "b"):
        C, S, L, B = fx[f"{c}:dims"].tolist()
        P = {k: v.double() for k, v in VR.vae_init(C, S, L, int(fx[f"{c}:seed"])).items()}
        x, eps = torch.from_numpy(fx[f"{c}:x"]).double(), torch.from_numpy(fx[f"{c}:eps"]).double()
        o, tape = VR.forward(P, x, eps, kw)
        margin = VR.kink_margin(tape)
        assert margin >= 1e-5 and abs(margin - float(fx[f"{c}:kink_margin"])) < 1e-12
        assert 1e-5 >= 10 * float(fx[f"{c}:f32_distance"])
        for key, ref in (("mu", o["mu"]), ("log_var", o["log_var"]), ("x_hat", o["x_hat"]), ("loss", o["loss"]),
                         ("recon", o["recon"]), ("kld", o["kld"])):
            got = torch.from_numpy(fx[f"{c}:{key}"]).double().reshape(ref.shape)
            assert float((got - ref).norm() / ref.norm()) < 1e-5, (c, key)
        for n, g in VR.backward(P, tape, kw).items():
            assert VR.fixture_grad_error(fx, c, n, g) < 1e-5, (c, n)


@pytest.mark.parametrize("shape", VR.DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_float32_scores_of_the_dense_shapes_stay_under_the_reference_worst(shape):
    B, K, N = shape
    for kind in ("xy", "yx", "wgrad"):
        p = bounds.Problem(kind, (B, 1, 1, K, N, 1, 1, 0))
        got = p.eval32()
        assert p.score(got) < bounds.C_REF_WORST, (kind, p.score(got))
        for name, bad in p.mutations(got).items():
            assert p.score(bad) > bounds.tolerance(p.n), (kind, name, p.score(bad), bounds.tolerance(p.n))
