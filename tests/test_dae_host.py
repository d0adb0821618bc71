"""The denoising autoencoder without a GPU: the loader and the shipped config, the module's surface against the reference's
(keys and shapes from the fixture), tests/dae_ref.py and the CPU module against tests/golden/dae.npz (tools/make_golden_dae.py),
the numpy restatement of the Philox mask against its statistics and its edges, the fixture's kink margin, and the float32 CPU
score of every dense shape with ReLU (so the bound tests/test_hip_dae.py holds the kernels to is one the reference's own
float32 meets)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import dae_ref as DR
import vae_ref as VR
from oracle import bounds

ENTRY_POINTS = ("lgm_dae_corrupt", "lgm_dae_mask_threshold", "lgm_dae_corrupt_mask", "lgm_dae_tanh_mse_fwd",
                "lgm_dae_tanh_mse_bwd", "lgm_dae_loss")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "lightning-generative-models_amd", "configs", "autoencoder", "dae.json")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dae.npz")))


def _dae(**kw):
    from models.generative.autoencoder.dae import DAE
    return DAE(**kw)


def _case(fx, c):
    C, S, B = fx[f"{c}:dims"].tolist()
    P = DR.dae_init(C, S, int(fx[f"{c}:seed"]))
    return (C, S, B), P, torch.from_numpy(fx[f"{c}:x"]), torch.from_numpy(fx[f"{c}:draws"]), str(fx[f"{c}:noise_type"]), \
        float(fx[f"{c}:level"])


def test_loader_builds_the_dae_from_the_shipped_config(fx):
    from utils.loader import load_config, load_model
    from models.generative.autoencoder.dae import DAE
    cfg = load_config(CONFIG)
    assert cfg["dataset"]["name"] == "MNIST" and cfg["dataset"]["batch_size"] == 32 and cfg["dataset"]["train_val_split"] == 0.8
    m = load_model(cfg["model"])
    assert type(m) is DAE and m.noise_type == "gaussian" and m.noise_level == 0.1
    keys = fx["keys"].tolist()
    assert list(m.state_dict().keys()) == keys == DR.KEYS
    assert [n for n, _ in m.named_parameters()] == keys
    for k, v in m.state_dict().items():
        assert list(v.shape) == fx[f"a:shape:{k}"].tolist(), k
    opt = m.configure_optimizers()
    assert type(opt) is torch.optim.Adam and opt.defaults["lr"] == 1e-3 and opt.defaults["betas"] == (0.9, 0.999)
    assert opt.defaults["weight_decay"] == 0.0
    assert m.prepare_hip("cpu") is None and m._flat is None          # a no-op on the CPU


def test_header_prototypes_exported_symbols_and_argument_checks():
    from lgm_hip import _lib
    from lgm_hip._lib import LgmArgumentError
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in protos, f"{name} is not declared in include/lgm_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert _lib.ABI_VERSION == 8
    L = _lib.lib()
    P = 4096                     # a non-null, 16-byte aligned address that is never dereferenced: every call is refused first
    for bad in ((None, 8, P, 8, 0.1, 2, 8, P, 8), (P, 7, P, 8, 0.1, 2, 8, P, 8), (P, 8, P, 8, 0.1, 0, 8, P, 8),
                (P, 8, P, 8, 0.1, 2, 7, P, 7), (P, 8, P, 8, 0.1, 2, 8, P + 64, 7), (P, 8, P + 64, 8, 0.1, 2, 8, P, 8)):
        with pytest.raises(LgmArgumentError):
            L.lgm_dae_corrupt(*bad, None)
    for bad in ((P, 8, None, 0, 0.1, 2, 8, P + 64, 8), (P, 8, P, 2, 0.1, 2, 8, P + 64, 8), (P, 8, P, 0, -0.1, 2, 8, P + 64, 8),
                (P, 8, P, 1, float("nan"), 2, 8, P + 64, 8), (P, 8, P, 0, 0.1, 2, 8, P, 8)):
        with pytest.raises(LgmArgumentError):
            L.lgm_dae_corrupt_mask(*bad, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_tanh_mse_fwd(P, 63, P + 1024, 64, 2, 64, P + 2048, 64, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_tanh_mse_bwd(P, 64, P + 1024, 64, None, 2, 64, P + 2048, 64, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_loss(P, 0, 64, P, None)
    # an output that overlaps an input at an offset, and more elements than the one-wave grids hold
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_corrupt(P, 8, P + 4096, 8, 0.1, 2, 8, P + 16, 8, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_corrupt_mask(P + 32, 8, P + 4096, 0, 0.1, 2, 8, P, 8, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_tanh_mse_bwd(P, 64, P + 1024, 64, P + 8192, 2, 64, P + 1024 + 256, 64, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_loss(P, 1 << 20, 1 << 20, P, None)
    with pytest.raises(LgmArgumentError):
        L.lgm_dae_corrupt(P, 1 << 20, P + (1 << 40), 1 << 20, 0.1, 1 << 12, 1 << 20, P + (1 << 41), 1 << 20, None)
    # relu joins the dense section's activations; SiLU and GELU stay out
    with pytest.raises(LgmArgumentError) as e:
        L.lgm_dense_fwd(P, 8, P, P, 2, 8, 8, 1, 0.0, P + 1024, 8, None, 0, None)
    assert "ReLU" in str(e.value)
    # thresholds, host-only
    assert L.lgm_dae_mask_threshold(0, 0.1) == DR.mask_threshold("salt_and_pepper", 0.1) == math.floor(0.05 * 2 ** 32)
    assert L.lgm_dae_mask_threshold(1, 0.1) == DR.mask_threshold("masking", 0.1) == math.floor(0.1 * 2 ** 32)
    assert L.lgm_dae_mask_threshold(0, 0.0) == 0 and L.lgm_dae_mask_threshold(0, 2.0) == 2 ** 32 - 1
    assert L.lgm_dae_mask_threshold(1, 1.0) == 2 ** 32 - 1 and L.lgm_dae_mask_threshold(2, 0.1) == -1


@pytest.mark.parametrize("c", ["a", "b"])
def test_float32_restatement_and_cpu_module_reproduce_the_fixture(fx, c):
    (C, S, B), P, x, draws, noise_type, level = _case(fx, c)
    want_xc = torch.from_numpy(fx[f"{c}:corrupted"])
    xc = DR.corrupt(x, noise_type, level, draws)
    assert torch.equal(xc, want_xc), "the restated corruption, in float32, to the bit"
    o, tape = DR.forward(P, x, xc)
    G = DR.backward(P, tape)
    m = _dae(img_channels=C, img_size=S, noise_type=noise_type, noise_level=level)
    m.load_state_dict(P)
    m.train()
    assert torch.equal(m.corrupt(x, noise=draws), want_xc)
    loss = m.training_step((x, None), 0, corrupted=m.corrupt(x, noise=draws))
    loss.backward()
    assert torch.equal(m.logged["loss"], loss)
    xh_m = m.denoise(want_xc)
    assert tuple(xh_m.shape) == (B, C, S, S) and torch.equal(m(want_xc), xh_m) and torch.equal(m.decode(m.encode(want_xc)), xh_m)
    for what, got in (("restatement", (o["x_hat"], o["loss"], G)),
                      ("module", (xh_m, loss.detach(), {n: p.grad for n, p in m.named_parameters()}))):
        xh, ls, grads = got
        want = torch.from_numpy(fx[f"{c}:x_hat"]).double().reshape(B, -1)
        assert float((xh.double().reshape(B, -1) - want).norm() / want.norm()) < 1e-5, what
        assert abs(float(ls) - float(fx[f"{c}:loss"])) / float(fx[f"{c}:loss"]) < 1e-5, what
        for n in DR.KEYS:
            assert DR.fixture_grad_error(fx, c, n, grads[n]) < 1e-5, (what, n)


@pytest.mark.parametrize("c", ["a", "b"])
def test_float64_restatement_agrees_with_the_fixture(fx, c):
    (C, S, B), P, x, _, _, _ = _case(fx, c)
    P64 = {k: v.double() for k, v in P.items()}
    o, tape = DR.forward(P64, x.double(), torch.from_numpy(fx[f"{c}:corrupted"]).double())
    want = torch.from_numpy(fx[f"{c}:x_hat"]).double().reshape(B, -1)
    assert float((o["x_hat"] - want).norm() / want.norm()) < 1e-4
    assert abs(float(o["loss"]) - float(fx[f"{c}:loss"])) / float(fx[f"{c}:loss"]) < 1e-4
    for n, g in DR.backward(P64, tape).items():
        assert DR.fixture_grad_error(fx, c, n, g) < 1e-4, n


@pytest.mark.parametrize("dims", [(1, 8, 4), (3, 5, 3)])
def test_dae_ref_against_float64_autograd(dims):
    C, S, B = dims
    P = {k: v.double() for k, v in DR.dae_init(C, S, 7).items()}
    m = _dae(img_channels=C, img_size=S).double()
    m.load_state_dict(P)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(B, C, S, S, generator=g).double() * 2 - 1
    xc = x + torch.randn(B, C, S, S, generator=g).double() * 0.1
    xh = m.decoder(m.encoder(xc))
    loss = m.metric(x, xh)
    (2.5 * loss).backward()
    o, tape = DR.forward(P, x, xc)
    G = DR.backward(P, tape, gloss=2.5)
    assert abs(float(o["loss"] - loss.detach())) < 1e-12
    assert float((o["x_hat"].view_as(xh) - xh.detach()).abs().max()) < 1e-12
    for n, p in m.named_parameters():
        assert float((G[n] - p.grad).abs().max()) < 1e-12, n


def test_numpy_mask_statistics_and_edges():
    B, D, key = 4, 784, 0x1234_5678_9ABC_DEF1
    n = B * D
    x = (np.random.RandomState(0).uniform(0.1, 0.9, size=(B, D))).astype(np.float32)      # neither 0 nor 1
    ws, wp = DR.mask_words(n, key)
    # the words against dropout_ref's own layout of the same counters (pass = the third counter word)
    import dropout_ref as DO
    assert np.array_equal(ws, DO.words((1, 1, n), key, 0, 0).reshape(-1))
    assert np.array_equal(wp, DO.words((1, 1, n), key, 1, 0).reshape(-1))
    for level in (0.1, 0.5):
        thr = DR.mask_threshold("salt_and_pepper", level)
        p = thr / 2.0 ** 32
        out = DR.corrupt_mask(x, key, "salt_and_pepper", level)
        pepper = (out == 0).mean()
        salt_drawn = (ws.reshape(B, D) < thr).mean()           # salt as drawn: pepper overwrites a few
        slack = 5 * math.sqrt(p * (1 - p) / n)
        assert abs(pepper - p) <= slack and abs(salt_drawn - p) <= slack, (level, pepper, salt_drawn, p)
        both = (ws < thr) & (wp < thr)
        assert bool((out.reshape(-1)[both] == 0).all()), "pepper wins where both hit, and pepper is 0"
        assert np.array_equal((out == 1), ((ws < thr) & ~(wp < thr)).reshape(B, D))
        keep = (out != 0) & (out != 1)
        assert np.array_equal(out[keep].view(np.uint32), x[keep].view(np.uint32))
        thr_m = DR.mask_threshold("masking", level)
        pm = thr_m / 2.0 ** 32
        outm = DR.corrupt_mask(x, key, "masking", level)
        assert abs((outm == 0).mean() - pm) <= 5 * math.sqrt(pm * (1 - pm) / n)
        assert not (outm == 1).any()
    for mode in DR.MODES:
        assert np.array_equal(DR.corrupt_mask(x, key, mode, 0.0).view(np.uint32), x.view(np.uint32)), "level 0 corrupts nothing"
    out = DR.corrupt_mask(x, key, "salt_and_pepper", 2.0)
    untouched = out.reshape(-1) == x.reshape(-1)
    assert np.array_equal(untouched, (ws == 2 ** 32 - 1) & (wp == 2 ** 32 - 1))
    assert DR.mask_threshold("salt_and_pepper", 2.0) == 2 ** 32 - 1 == DR.mask_threshold("masking", 7.0)
    # a straddling row length: the result is defined by the logical index alone
    x3 = x.reshape(-1)[:3 * 75].reshape(3, 75)
    assert np.array_equal(DR.corrupt_mask(x3, key, "masking", 0.3).reshape(-1),
                          DR.corrupt_mask(x3.reshape(1, -1), key, "masking", 0.3).reshape(-1))


def _relu_scores(shape):
    """forward_error_units of torch's float32 CPU results with ReLU: y, gx, (gw, gb)"""
    B, K, N = shape
    t = bounds.Problem("wgrad", (B, 1, 1, K, N, 1, 1, 0)).t
    x, w, gy = t["x"].view(B, K), t["w"].view(N, K), t["gy"].view(B, N)
    gw0, gb0 = t["gw0"].view(N, K), t["gb0"]
    b = bounds.Problem("xy", (B, 1, 1, K, N, 1, 1, 0)).t["b"]
    pre = x.double() @ w.double().T + b.double()
    S = x.abs().double() @ w.abs().double().T + b.abs().double()
    y32 = torch.relu(torch.nn.functional.linear(x, w, b))
    out = {"y": bounds.forward_error_units(y32, torch.relu(pre), S)}
    y = torch.relu(torch.randn(B, N, generator=torch.Generator().manual_seed(B + K + N)) + 0.3)     # a saved output
    live = y > 0
    g32 = gy * live
    g64 = gy.double() * live
    out["gx"] = bounds.forward_error_units(g32 @ w, g64 @ w.double(), g64.abs() @ w.abs().double())
    got = torch.cat([(gw0 + g32.T @ x).reshape(-1), gb0 + g32.sum(0)])
    ref = torch.cat([(gw0.double() + g64.T @ x.double()).reshape(-1), gb0.double() + g64.sum(0)])
    Sg = torch.cat([(gw0.abs().double() + g64.abs().T @ x.abs().double()).reshape(-1), gb0.abs().double() + g64.abs().sum(0)])
    out["gw, gb"] = bounds.forward_error_units(got, ref, Sg)
    return out


@pytest.mark.parametrize("shape", VR.DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_float32_scores_with_relu_stay_under_the_reference_worst(shape):
    for what, score in _relu_scores(shape).items():
        assert score < bounds.C_REF_WORST, (what, score)


def test_fixture_holds_its_kink_margin(fx):
    assert fx["cases"].tolist() == ["a", "b"]
    assert [fx[f"{c}:dims"].tolist() for c in ("a", "b")] == [[1, 28, 4], [1, 28, 3]]
    assert [str(fx[f"{c}:noise_type"]) for c in ("a", "b")] == ["gaussian", "salt_and_pepper"]
    for c in ("a", "b"):
        (C, S, B), P, x, _, _, _ = _case(fx, c)
        P64 = {k: v.double() for k, v in P.items()}
        _, tape = DR.forward(P64, x.double(), torch.from_numpy(fx[f"{c}:corrupted"]).double())
        margin = DR.kink_margin(tape)
        assert margin >= 1e-5 and abs(margin - float(fx[f"{c}:kink_margin"])) < 1e-12
        assert 1e-5 >= 10 * float(fx[f"{c}:f32_distance"])


def test_unknown_noise_type_and_wrong_shapes_raise():
    with pytest.raises(ValueError):
        _dae(noise_type="speckle")
    m = _dae(img_channels=1, img_size=8)
    m.noise_type = "speckle"                                  # set after construction, as the reference allows
    with pytest.raises(ValueError):
        m.training_step((torch.zeros(2, 1, 8, 8), None), 0)
    with pytest.raises(ValueError):
        DR.corrupt(torch.zeros(1), "speckle", 0.1, None)
    m = _dae(img_channels=1, img_size=8, noise_type="masking", noise_level=0.5)
    x = torch.rand(3, 1, 8, 8) * 0.8 + 0.1
    u = torch.rand(3, 1, 8, 8)
    assert torch.equal(m.corrupt(x, noise=u), torch.where(u < 0.5, torch.zeros_like(x), x))
    for bad in (torch.zeros(3, 64), torch.zeros(3, 1, 8, 7), torch.zeros(3, 3, 8, 8)):
        with pytest.raises(ValueError):
            m.encode(bad)
        with pytest.raises(ValueError):
            m.corrupt(bad)
        with pytest.raises(ValueError):
            m.training_step((bad, None), 0)
    for bad in (torch.zeros(3, 127), torch.zeros(128), torch.zeros(3, 128, 1)):
        with pytest.raises(ValueError):
            m.decode(bad)
    with pytest.raises(ValueError):
        m.corrupt(x, key=3)                                    # a Philox key belongs to the GPU path
    assert tuple(m.encode(x).shape) == (3, 128) and tuple(m.decode(m.encode(x)).shape) == (3, 1, 8, 8)
