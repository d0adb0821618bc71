"""The MLP GAN without a GPU: the library's new symbols and their argument checks, the module's surface against the
reference's (keys and parameter order written out), the CPU path against a plain torch restatement to the bit,
tests/gan_ref.py against float64 autograd, every refusal, the config, the fixture's margins, the float64 side of the
centred-variance claim that tests/test_hip_gan_mlp.py makes on the device, and the subclasses left as they were."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch
from torch import nn

import gan_ref as GR

ENTRY_POINTS = ("lgm_bn1d_supported", "lgm_bn1d_fwd", "lgm_bn1d_bwd", "lgm_gan_bce_d", "lgm_gan_bce_g", "lgm_gan_bce_bwd",
                "lgm_dense_dgrad")

# reference models/generative/gan/gan.py:35-47, :78-84 - written out, not derived
_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
REF_G_KEYS = (["model.0.weight", "model.0.bias"] + [f"model.1.{p}" for p in _BN] + ["model.3.weight", "model.3.bias"]
              + [f"model.4.{p}" for p in _BN] + ["model.6.weight", "model.6.bias"] + [f"model.7.{p}" for p in _BN]
              + ["model.9.weight", "model.9.bias"])
REF_D_KEYS = ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.4.weight", "model.4.bias"]
REF_PARAMS = (["G.model.0.weight", "G.model.0.bias", "G.model.1.weight", "G.model.1.bias", "G.model.3.weight", "G.model.3.bias",
               "G.model.4.weight", "G.model.4.bias", "G.model.6.weight", "G.model.6.bias", "G.model.7.weight", "G.model.7.bias",
               "G.model.9.weight", "G.model.9.bias"] + [f"D.{k}" for k in REF_D_KEYS])
REF_SHAPES = {"G.model.0.weight": (256, 100), "G.model.1.weight": (256,), "G.model.1.running_var": (256,),
              "G.model.1.num_batches_tracked": (), "G.model.3.weight": (512, 256), "G.model.4.bias": (512,),
              "G.model.6.weight": (1024, 512), "G.model.7.running_mean": (1024,), "G.model.9.weight": (784, 1024),
              "G.model.9.bias": (784,), "D.model.0.weight": (512, 784), "D.model.2.weight": (256, 512),
              "D.model.4.weight": (1, 256), "D.model.4.bias": (1,)}

# sha256 over the float32 bytes of DCGAN(1, 28, 100, ...).state_dict() after torch.manual_seed(1234), in key order, and the
# first draw after construction - recorded from the commit before the MLP pair existed
DCGAN_SEED = 1234
DCGAN_STATE_SHA = "adf838c2e6497866f4aaef74eb753bcb3591b7ffeaee67d74376cd12af6fa358"
DCGAN_NEXT_DRAW = "0.8163132071495056"


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "gan_mlp.npz")))


def _lib():
    from lgm_hip import _lib
    return _lib.lib()


def _gan(*a, **kw):
    from models.generative.gan.gan import GAN
    return GAN(*a, **kw)


def _with_optimizers(m):
    from lgm_hip.lightning import _CountingOptimizer
    opts, _ = m.configure_optimizers()
    m._optimizers = [_CountingOptimizer(o, m) for o in opts]
    return opts


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
    assert L.lgm_bn1d_supported(2, 4) == 1 and L.lgm_bn1d_supported(512, 1024) == 1
    assert L.lgm_bn1d_supported(513, 4) == 0 and L.lgm_bn1d_supported(0, 4) == 0 and L.lgm_bn1d_supported(4, 0) == 0

    def fwd(a=P, ap=8, B=4, F=6, gm=P, bt=P, training=1, act=4, rm=P, rv=P, y=2 * P, yp=8, mean=P, rstd=P):
        L.lgm_bn1d_fwd(a, ap, B, F, gm, bt, 1e-5, 0.1, training, act, 0.2, rm, rv, y, yp, mean, rstd, None)
    for bad in (dict(a=None), dict(gm=None), dict(bt=None), dict(rm=None), dict(rv=None), dict(y=None), dict(mean=None),
                dict(rstd=None), dict(B=0), dict(B=513), dict(F=0), dict(ap=5), dict(yp=7), dict(act=5), dict(act=3),
                dict(B=1), dict(y=P)):                     # B = 1 in training mode; y aliasing a
        with pytest.raises(LgmArgumentError):
            fwd(**bad)

    def bwd(gy=P, gyp=8, y=P, yp=8, a=P, ap=8, mean=P, rstd=P, gm=P, B=4, F=6, act=4, ga=P, gap=8, gg=P, gb=P):
        L.lgm_bn1d_bwd(gy, gyp, y, yp, a, ap, mean, rstd, gm, B, F, act, 0.2, ga, gap, gg, gb, 0.0, None)
    for bad in (dict(gy=None), dict(a=None), dict(mean=None), dict(rstd=None), dict(gm=None), dict(ga=None), dict(gg=None),
                dict(gb=None), dict(y=None), dict(B=0), dict(B=600), dict(gyp=5), dict(ap=5), dict(yp=5), dict(gap=7),
                dict(act=5)):
        with pytest.raises(LgmArgumentError):
            bwd(**bad)
    for bad in ((None, 4, P, 4, 3, P), (P, 4, None, 4, 3, P), (P, 4, P, 4, 3, None), (P, 4, P, 4, 0, P), (P, 0, P, 4, 3, P)):
        with pytest.raises(LgmArgumentError):
            L.lgm_gan_bce_d(*bad, None)
    for bad in ((None, 4, 3, 0, P), (P, 4, 3, 0, None), (P, 4, 0, 0, P), (P, 4, 3, 2, P), (P, 0, 3, 0, P)):
        with pytest.raises(LgmArgumentError):
            L.lgm_gan_bce_g(*bad, None)
    for bad in ((None, 4, 1.0, 1.0, P, 4, None, 0, 0.0, 0.0, None, 0, 3, P), (P, 4, 1.0, 1.0, None, 4, None, 0, 0.0, 0.0, None, 0, 3, P),
                (P, 4, 1.0, 1.0, P, 4, None, 0, 0.0, 0.0, None, 0, 3, None), (P, 4, 1.0, 1.0, P, 3, None, 0, 0.0, 0.0, None, 0, 3, P),
                (P, 4, 0.5, 1.0, P, 4, None, 0, 0.0, 0.0, None, 0, 3, P), (P, 4, 1.0, 1.0, P, 4, P, 4, 0.0, 0.5, None, 0, 3, P),
                (P, 4, 1.0, 1.0, P, 4, None, 0, 0.0, 0.0, None, 0, 0, P)):
        with pytest.raises(LgmArgumentError):
            L.lgm_gan_bce_bwd(*bad, None)
    nb = L.lgm_dense_bwd_workspace(2, 8, 8, 1)
    for bad in ((None, 8, P, 8, P, 2, 8, 8, 4, 0.2, P, 8, P, nb), (P, 8, None, 8, P, 2, 8, 8, 4, 0.2, P, 8, P, nb),
                (P, 8, P, 8, None, 2, 8, 8, 4, 0.2, P, 8, P, nb), (P, 8, P, 8, P, 2, 8, 8, 4, 0.2, None, 8, P, nb),
                (P, 8, P, 8, P, 2, 8, 8, 4, 0.2, P, 8, None, nb), (P, 8, P, 8, P, 2, 8, 8, 4, 0.2, P, 8, P, nb - 4),
                (P, 7, P, 8, P, 2, 8, 8, 4, 0.2, P, 8, P, nb), (P, 8, P, 8, P, 2, 8, 8, 4, 0.2, P, 7, P, nb),
                (P, 8, P, 8, P, 0, 8, 8, 4, 0.2, P, 8, P, nb), (P, 8, P, 8, P, 2, 8, 8, 2, 0.2, P, 8, P, nb)):
        with pytest.raises(LgmArgumentError):
            L.lgm_dense_dgrad(*bad, None)


def test_module_surface_keys_shapes_and_parameter_order():
    from models.generative.gan.gan import Discriminator, Generator
    m = _gan(1, 28, 100)
    assert type(m.G) is Generator and type(m.D) is Discriminator
    assert list(m.G.state_dict().keys()) == REF_G_KEYS == GR.G_KEYS
    assert list(m.D.state_dict().keys()) == REF_D_KEYS == GR.D_KEYS
    assert list(m.state_dict().keys()) == [f"G.{k}" for k in REF_G_KEYS] + [f"D.{k}" for k in REF_D_KEYS]
    assert [n for n, _ in m.named_parameters()] == REF_PARAMS
    sd = m.state_dict()
    for k, shape in REF_SHAPES.items():
        assert tuple(sd[k].shape) == shape, k
    assert sd["G.model.1.num_batches_tracked"].dtype == torch.long
    assert m.G.img_shape == [1, 28, 28] and m.G.latent_dim == 100 and m.G.device == torch.device("cpu")
    assert tuple(m.z.shape) == (64, 100) and m.automatic_optimization is False
    for name in ("make_fast_step", "sample", "prepare_hip", "forward", "training_step", "validation_step"):
        assert callable(getattr(m, name)), name
    assert callable(Generator.random_sample)
    m.prepare_hip("cpu")
    assert m.G._flat is None and m.D._flat is None                   # a no-op on the CPU
    assert all(type(p) is nn.Parameter and not hasattr(p, "_lgm_flat") for p in m.parameters())
    opts, scheds = m.configure_optimizers()
    assert [type(o) for o in opts] == [torch.optim.Adam, torch.optim.Adam] and scheds == []
    assert [id(p) for p in opts[0].param_groups[0]["params"]] == [id(p) for p in m.D.parameters()]
    assert opts[0].defaults["betas"] == (0.5, 0.999) and opts[0].defaults["weight_decay"] == 1e-5
    assert tuple(m.G.random_sample(3).shape) == (3, 1, 28, 28) and tuple(m(torch.zeros(2, 100)).shape) == (2, 1, 28, 28)
    assert tuple(m.D(torch.zeros(3, 1, 28, 28)).shape) == (3,) and tuple(m.D(torch.zeros(1, 1, 28, 28)).shape) == ()


def test_every_refusal():
    from lgm_hip.bn import BatchNorm1d
    with pytest.raises(ValueError):
        _gan(1, 8, 4, loss_type="hinge")
    with pytest.raises(ValueError):
        _gan(1, 8, 4, loss_type="")
    m = _gan(1, 8, 4)
    for z in (torch.zeros(3, 5), torch.zeros(4), torch.zeros(3, 4, 1), torch.zeros(2, 4)):
        with pytest.raises(ValueError):
            m.sample(3, z=z)
    bn = BatchNorm1d(6)
    bn.train()
    with pytest.raises(ValueError):
        bn(torch.zeros(1, 6))
    with pytest.raises(ValueError):
        bn.fwd(torch.zeros(1, 6))                                     # refused before anything touches a device
    bn.eval()
    assert tuple(bn(torch.zeros(1, 6)).shape) == (1, 6)
    z = torch.randn(3, 4)
    m.eval()
    assert torch.equal(m.sample(3, z=z), m.G(z).detach()) and tuple(m.sample(5).shape) == (5, 1, 8, 8)


def _plain_torch_gan(C, S, L):
    """the reference's two networks in its construction order"""
    D = C * S * S
    G = nn.Sequential(nn.Linear(L, 256), nn.BatchNorm1d(256), nn.LeakyReLU(0.2), nn.Linear(256, 512), nn.BatchNorm1d(512),
                      nn.LeakyReLU(0.2), nn.Linear(512, 1024), nn.BatchNorm1d(1024), nn.LeakyReLU(0.2), nn.Linear(1024, D),
                      nn.Tanh())
    Dn = nn.Sequential(nn.Linear(D, 512), nn.LeakyReLU(0.2), nn.Linear(512, 256), nn.LeakyReLU(0.2), nn.Linear(256, 1))
    return G, Dn


@pytest.mark.parametrize("loss_type", GR.LOSS_TYPES)
def test_cpu_path_is_bit_equal_to_a_plain_torch_restatement(loss_type):
    C, S, L, B = 1, 8, 6, 5
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    kw = dict(lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-5)
    torch.manual_seed(11)
    m = _gan(C, S, L, lr=1e-2, loss_type=loss_type)
    after_m = torch.rand(1)
    torch.manual_seed(11)
    G, Dn = _plain_torch_gan(C, S, L)
    z64 = torch.randn([64, L])
    assert torch.equal(torch.rand(1), after_m), "the constructor draws what the reference's draws, no more"
    assert torch.equal(m.z, z64)
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), list(G.parameters()) + list(Dn.parameters())))
    _with_optimizers(m)
    m.train()
    d_opt, g_opt = torch.optim.Adam(Dn.parameters(), **kw), torch.optim.Adam(G.parameters(), **kw)
    x = torch.rand(B, C, S, S, generator=torch.Generator().manual_seed(3)) * 2 - 1
    for step in range(2):
        torch.manual_seed(5 + step)
        logs = m.training_step((x, None))
        torch.manual_seed(5 + step)
        x_hat = G(torch.randn([B, L])).view(-1, C, S, S)
        s_r, s_f = Dn(x.view(B, -1)).squeeze(), Dn(x_hat.detach().view(B, -1)).squeeze()
        real, fake = bce(s_r, torch.ones_like(s_r)), bce(s_f, torch.zeros_like(s_f))
        d_loss = (real + fake) / 2
        d_opt.zero_grad(set_to_none=True)
        d_loss.backward()
        d_opt.step()
        s = Dn(x_hat.view(B, -1)).squeeze()
        g_loss = -bce(s, torch.zeros_like(s)) if loss_type == "min-max" else bce(s, torch.ones_like(s))
        g_opt.zero_grad(set_to_none=True)
        g_loss.backward()
        g_opt.step()
        want = {"train_d_loss": d_loss, "train_d_loss_real": real, "train_d_loss_fake": fake, "train_logits_real": s_r.mean(),
                "train_logits_fake": s.mean(), "train_g_loss": g_loss}
        assert set(logs) == set(want) and all(torch.equal(logs[k], want[k]) for k in want), step
        assert all(torch.equal(m.logged[k], want[k]) for k in want)
    assert m.global_step == 4
    got, ref = m.state_dict(), {**{f"G.model.{k}": v for k, v in G.state_dict().items()}, **{f"D.model.{k}": v for k, v in Dn.state_dict().items()}}
    assert list(got) == list(ref) and all(torch.equal(got[k], ref[k]) for k in ref)
    assert int(got["G.model.1.num_batches_tracked"]) == 2
    m.eval()
    G.eval()
    with torch.no_grad():
        m.validation_step((x, None))
    assert "val_d_loss" in m.logged and m.global_step == 4 and int(m.state_dict()["G.model.1.num_batches_tracked"]) == 2


@pytest.mark.parametrize("dims", [(1, 8, 6, 5), (3, 5, 3, 4)])
def test_gan_ref_against_float64_autograd(dims):
    C, S, L, B = dims
    P = GR.to64(GR.gan_init(C, S, L, 7))
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    g = torch.Generator().manual_seed(8)
    x, z = torch.rand(B, C, S, S, generator=g).double() * 2 - 1, torch.randn(B, L, generator=g).double()
    for lt in GR.LOSS_TYPES:
        m = _gan(C, S, L, loss_type=lt).double()
        m.load_state_dict(P)
        m.train()
        x_hat = m.G(z)
        xh, tape, running = GR.g_forward(P, z, True)
        assert float((xh - x_hat.detach().reshape(B, -1)).abs().max()) < 1e-12
        sd = m.G.state_dict()
        for k, v in running.items():
            assert float((v - sd[k[2:]]).abs().max()) < 1e-12, k
        assert int(sd["model.4.num_batches_tracked"]) == 1
        d = m._calculate_d_loss(x, x_hat)
        (2.5 * d["d_loss"]).backward()
        out, GD = GR.d_loss(P, x, xh, gloss=2.5)
        for k in ("d_loss", "d_loss_real", "d_loss_fake", "logits_real", "logits_fake"):
            assert abs(float(out[k] - d[k].detach())) < 1e-12, k
        for n, p in m.D.named_parameters():
            assert float((GD[n] - p.grad).abs().max()) < 1e-12, n
        m.zero_grad(set_to_none=True)
        gl = m._calculate_g_loss(x_hat)
        (0.5 * gl["g_loss"]).backward()
        loss, mean_s, _, gxh = GR.g_loss(P, xh, lt, gloss=0.5)
        assert abs(float(loss - gl["g_loss"].detach())) < 1e-12 and abs(float(mean_s - gl["logits_fake"].detach())) < 1e-12
        for n, gr in GR.g_backward(P, tape, gxh).items():
            ref = dict(m.G.named_parameters())[n].grad
            assert float((gr - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max())), (lt, n)
        # eval mode: the running statistics normalise and do not move
        m.eval()
        xe = m.G(z).detach().reshape(B, -1)
        P1 = {**P, **running}
        assert float((GR.g_forward(P1, z, False)[0] - xe).abs().max()) < 1e-12
    s = torch.tensor([-40.0, -1.5, 0.0, 2.0, 40.0], dtype=torch.float64)
    for t in (0.0, 1.0):
        assert float((GR.bce(s, t) - bce(s, torch.full_like(s, t), reduction="none")).abs().max()) < 1e-15


def test_config_loads_through_the_loader():
    from models.generative.gan.gan import GAN
    from utils.loader import load_config, load_model
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lightning-generative-models_amd")
    cfg = load_config(os.path.join(pkg, "configs", "gan", "gan.json"))
    assert cfg["dataset"] == {"batch_size": 32, "img_channels": 1, "img_size": 28, "name": "MNIST", "train_val_split": 0.8}
    assert cfg["model"]["name"] == "GAN"
    assert cfg["model"]["args"] == {"b1": 0.5, "b2": 0.999, "img_channels": 1, "img_size": 28, "latent_dim": 100,
                                    "loss_type": "non-saturating", "lr": 1e-4, "weight_decay": 1e-5}
    m = load_model(cfg["model"])
    assert type(m) is GAN and m.hparams.loss_type == "non-saturating" and m.hparams.lr == 1e-4
    assert list(m.state_dict().keys()) == GR.KEYS


def test_fixture_holds_its_margins_and_agrees_with_gan_ref(fx):
    assert fx["cases"].tolist() == ["a", "b"] and fx["loss_types"].tolist() == list(GR.LOSS_TYPES)
    assert [fx[f"{c}:dims"].tolist() for c in ("a", "b")] == [[1, 8, 6, 5], [3, 5, 3, 4]]
    for c in ("a", "b"):
        C, S, L, B = fx[f"{c}:dims"].tolist()
        P = GR.to64(GR.gan_init(C, S, L, int(fx[f"{c}:seed"])))
        x, z = torch.from_numpy(fx[f"{c}:x"]).double(), torch.from_numpy(fx[f"{c}:z"]).double()
        margin = float(GR.kink_values(P, z, x).abs().min())
        assert margin >= 1e-5 and abs(margin - float(fx[f"{c}:kink_margin"])) < 1e-12
        assert margin >= 10 * float(fx[f"{c}:f32_distance"])
        xh, tape, running = GR.g_forward(P, z, True)
        out, GD = GR.d_loss(P, x, xh)

        def close(key, ref):
            got = torch.from_numpy(fx[f"{c}:{key}"]).double().reshape(ref.shape)
            assert float((got - ref).norm() / ref.norm()) < 1e-5, (c, key)
        close("x_hat", xh.reshape(B, C, S, S))
        close("s_real", out["s_real"])
        close("s_fake", out["s_fake"])
        for k in ("d_loss", "d_loss_real", "d_loss_fake", "logits_real", "logits_fake"):
            close(k, out[k])
        for k, v in running.items():
            close(k, v)
        for n, g in GD.items():
            assert GR.fixture_grad_error(fx, c, f"D.{n}", g) < 1e-5, (c, n)
        for lt in GR.LOSS_TYPES:
            loss, _, _, gxh = GR.g_loss(P, xh, lt)
            close(f"g_loss:{lt}", loss)
            G = GR.g_backward(P, tape, gxh)
            for n, g in G.items():
                if n in ("model.0.bias", "model.3.bias", "model.6.bias"):
                    # analytically zero (the BatchNorm behind it removes the mean): absolute, against the layer's weights
                    stored = torch.from_numpy(fx[f"{c}:grad:G:{lt}:{n}"]).double()
                    assert float(stored.abs().max()) <= 1e-4 * float(G[n.replace("bias", "weight")].abs().max()), (c, lt, n)
                    assert float(g.abs().max()) <= 1e-12
                else:
                    assert GR.fixture_grad_error(fx, c, f"G:{lt}:{n}", g) < 1e-5, (c, lt, n)


def test_one_pass_variance_misses_the_bound_the_centred_form_holds():
    """The float64 side of the device test's input choice: column means of about 30 with unit spread.  Both variance forms
    are evaluated in float32 arithmetic on the CPU (sequential sums, every operation rounded) and scored as the device test
    scores y: |err| / ((k + 2) u M) with k = ceil(B / 16) + 18 and M = |gamma| rstd mean|a| + |gamma xhat| + |beta|."""
    B, F = 33, 36
    g = torch.Generator().manual_seed(5)
    a = (torch.randn(B, F, generator=g) + 30.0 + torch.randn(F, generator=g)).float()
    gamma, beta = torch.rand(F, generator=g) + 0.5, torch.rand(F, generator=g) - 0.5
    n64, xhat64, _, _, rstd64 = GR.bn_train(a.double(), gamma.double(), beta.double())
    M = gamma.double().abs() * rstd64 * a.double().abs().mean(0) + (gamma.double() * xhat64).abs() + beta.double().abs()
    k = -(-B // 16) + 18
    bound = (k + 2) * 2.0 ** -24 * M

    def seq_sum(t):
        s = torch.zeros(F)
        for b in range(B):
            s = s + t[b]
        return s
    mean = seq_sum(a) / B
    centred = seq_sum((a - mean) * (a - mean)) / B
    one_pass = seq_sum(a * a) / B - mean * mean
    scores = []
    for var in (centred, one_pass):
        y = gamma * ((a - mean) * (1.0 / torch.sqrt(var + 1e-5))) + beta
        scores.append(float(((y.double() - n64).abs() / bound).max()))
    assert scores[0] <= 1.0 < scores[1], scores


def _state_sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_subclasses_are_what_they_were():
    from models.generative.gan.dcgan import DCGAN
    from models.generative.gan.lsgan import LSGAN
    torch.manual_seed(DCGAN_SEED)
    m = DCGAN(1, 28, 100, 2e-4, 0.5, 0.999, 1e-5)
    nxt = torch.rand(1)
    assert _state_sha(m.state_dict()) == DCGAN_STATE_SHA
    assert repr(float(nxt)) == DCGAN_NEXT_DRAW, "the constructor draws what it drew"
    assert tuple(m.z.shape) == (16, 100, 1, 1)
    assert m.make_fast_step(None) is None and m.make_fast_step([None, None], 2, False) is None
    ls = LSGAN(1, 28, 100, 2e-4, 0.5, 0.999, 1e-5)
    assert ls.make_fast_step(None) is None
    from models.generative.gan.wgan import WGAN
    assert WGAN.make_fast_step is not DCGAN.make_fast_step
