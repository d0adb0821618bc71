"""CPU: the eps / x0 / v objectives and offset noise of GaussianDiffusion at the layers that need no GPU - the loss
weights against the reference's (tests/golden/diffusion_objectives.npz, written by tools/make_golden_objectives.py),
argument checking, the DDPM module's hyper-parameters, configs/diffusion/ddpm_eps.json and the C-ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lightning-generative-models_amd")
CFG = os.path.join(PKG, "configs", "diffusion", "ddpm_eps.json")
NEW_SYMBOLS = ("lgm_qsample_target_obj", "lgm_model_predictions_obj", "lgm_sample_step_obj", "lgm_sample_step_table_obj")


@pytest.mark.parametrize("min_snr", [False, True])
@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_loss_weight_matches_the_reference(golden_dir, objective, min_snr):
    """reference ddpm.py:649-662: bit-equal at the 12 indices of diffusion_schedule.npz, float64 sum within 1e-6."""
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    fx = np.load(os.path.join(golden_dir, "diffusion_objectives.npz"))
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, timesteps=1000, objective=objective,
                           min_snr_loss_weight=min_snr, min_snr_gamma=5)
    key = f"{objective}:loss_weight" + ("_minsnr" if min_snr else "")
    lw = gd.loss_weight
    assert lw.dtype == torch.float32 and lw.shape == (1000,)
    assert np.array_equal(lw[torch.as_tensor(fx["idx"])].numpy(), fx[key]), key
    want = float(fx[key + "__sum"])
    assert abs(lw.double().sum().item() - want) <= 1e-6 * abs(want), key
    if objective == "pred_noise" and not min_snr:
        assert torch.equal(lw, torch.ones(1000))
    if objective == "pred_x0" and min_snr:
        assert float(lw.max()) == 5.0


def test_unknown_objective_is_a_value_error():
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    with pytest.raises(ValueError, match="objective"):
        GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, objective="pred_score")
    gd = GaussianDiffusion(Unet(dim=16, channels=3), img_size=16, objective="pred_x0", offset_noise_strength=0.25)
    assert gd.objective == "pred_x0" and gd.offset_noise_strength == 0.25


def test_ddpm_module_takes_the_objective_and_keeps_it_in_hparams():
    from models.generative.diffusion.ddpm import DDPM
    m = DDPM(3, 16, 16, 1000, None, 1e-3, (0.9, 0.99), 10, 0.995, objective="pred_noise", offset_noise_strength=0.1,
             min_snr_loss_weight=True)
    hp = dict(m.hparams)
    assert hp["objective"] == "pred_noise" and hp["offset_noise_strength"] == 0.1 and hp["min_snr_loss_weight"] is True
    assert hp["beta_schedule"] == "sigmoid" and hp["min_snr_gamma"] == 5
    assert (hp["img_channels"], hp["img_size"], hp["dim"], hp["lr"], hp["ema_decay"]) == (3, 16, 16, 1e-3, 0.995)
    for gd in (m.ema.online_model, m.ema.ema_model):
        assert gd.objective == "pred_noise" and gd.offset_noise_strength == 0.1
        assert float(gd.loss_weight.max()) == 1.0 and float(gd.loss_weight.min()) < 1.0      # min(snr, 5) / snr
    again = DDPM(**hp)                                         # the hyper-parameters rebuild the module
    assert torch.equal(again.ema.online_model.loss_weight, m.ema.online_model.loss_weight)
    d = DDPM(img_size=16, dim=16)                              # defaults: the reference's
    assert d.hparams["objective"] == "pred_v" and d.hparams["offset_noise_strength"] == 0.0
    assert d.hparams["min_snr_loss_weight"] is False
    lin = DDPM(img_size=16, dim=16, beta_schedule="linear").ema.online_model
    assert abs(float(lin.betas[0]) - 1e-4) < 1e-9 and abs(float(lin.betas[-1]) - 0.02) < 1e-8


def test_ddpm_eps_config_loads_and_builds_the_model():
    from utils.loader import load_config, load_model
    c = load_config(CFG)
    a = c["model"]["args"]
    assert c["model"]["name"] == "DDPM" and a["img_size"] == c["dataset"]["img_size"] == 32 and a["dim"] == 64
    assert a["objective"] == "pred_noise" and a["min_snr_loss_weight"] is True and a["offset_noise_strength"] == 0.1
    assert c["dataset"] == load_config(os.path.join(PKG, "configs", "diffusion", "ddpm.json"))["dataset"]
    m = load_model(c["model"])
    gd = m.ema.online_model
    assert type(m).__name__ == "DDPM" and gd.objective == "pred_noise" and gd.offset_noise_strength == 0.1
    assert m.hparams["objective"] == "pred_noise"


def test_new_entry_points_are_declared_and_exported():
    from lgm_hip import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/lgm_hip.h"
        assert hasattr(dll, name), f"{name} is not exported by the library"
    assert len(protos["lgm_qsample_target_obj"][1]) == len(protos["lgm_qsample_target"][1]) + 3
    assert len(protos["lgm_sample_step_table_obj"][1]) == len(protos["lgm_sample_step_table"][1]) + 2
    # the host rejects an objective outside 0..2 before any launch (no GPU needed)
    L = _lib.lib()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    with pytest.raises(_lib.LgmArgumentError, match="sample_step_obj"):
        L.lgm_sample_step_obj(p, p, None, p, None, 1, 1, 1, 4, 3, 0.0, 0.0, 1, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, None)


class _Recorder:
    """Stands in for the library: records (entry point, arguments) of every call and answers 0 (launched)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lgm_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def recorder(monkeypatch):
    from lgm_hip import ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    monkeypatch.setattr(ops, "stream", lambda: 0)
    return rec


def _diffusion(objective, self_condition):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    return GaussianDiffusion(Unet(dim=16, channels=3, self_condition=self_condition), img_size=16, timesteps=1000,
                             objective=objective)


@pytest.mark.parametrize("self_condition", [False, True])
@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_q_sample_is_one_slice_launch_for_every_network(recorder, objective, self_condition):
    """hip_loss_qsample: one lgm_qsample_target_slice call whatever the objective, on the network's own buffer layout"""
    from models.generative.diffusion.ddpm import OBJECTIVES, hip_loss_qsample
    gd = _diffusion(objective, self_condition)
    net = gd.model
    assert (net.in_pitch, net.x_off, net.sc_off) == ((8, 3, 0) if self_condition else (4, 0, -1))
    img, noise = torch.rand(2, 3, 16, 16), torch.randn(2, 3, 16, 16)
    xt, target, *_ = hip_loss_qsample(gd, img, torch.tensor([3, 700]), noise, True)
    assert [name for name, _ in recorder.calls] == ["lgm_qsample_target_slice"]
    args = recorder.calls[0][1]
    assert args[8] == OBJECTIVES[objective]
    assert args[9] == xt.data_ptr() and args[10:13] == (net.in_pitch, net.x_off, net.sc_off)
    assert args[13] == target.data_ptr() and args[14:19] == (4, 2, 3, 256, 4)
    assert tuple(xt.shape) == (2, 16, 16, net.in_pitch) and tuple(target.shape) == (2, 16, 16, 4)


@pytest.mark.parametrize("self_condition", [False, True])
@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_eager_sampler_step_branches_on_where_x_start_goes(recorder, monkeypatch, objective, self_condition):
    """_Chain.step: lgm_sample_step_slice for a self-conditioned network (x_start into its slice), lgm_sample_step_obj with
    the x0 buffer otherwise - for every objective; the 8 scalars are the ones of the coefficient functions."""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import OBJECTIVES
    gd = _diffusion(objective, self_condition)
    net = gd.model
    monkeypatch.setattr(net, "prepare_hip", lambda device: None)
    monkeypatch.setattr(net, "forward_guided", lambda x, t, classes=None, cond_scale=1.0, **kw: torch.zeros(
        x.shape[:3] + (4,)))
    shape = (2, 3, 16, 16)
    for step, coeffs, rederive in (
            (lambda ch, nz: sampler.p_sample_step(ch, 500, nz), sampler._p_sample_coeffs(gd, 500), 0),
            (lambda ch, nz: sampler.ddim_step(ch, 999, 979, nz, 1.0), sampler._ddim_coeffs(gd, 999, 979, 1.0), 1)):
        chain = sampler._Chain(gd, shape, torch.randn(shape))
        x, x_next, x0, nz = chain.x, chain.x_next, chain.x0, torch.randn(shape)
        recorder.calls.clear()
        step(chain, nz)
        (name, args), = recorder.calls
        head, tail = (A, Bv), (R, Rm1, C0, C1, C2, C3) = coeffs[:2], coeffs[2:]
        assert C3 != 0.0
        if self_condition:
            assert name == "lgm_sample_step_slice"
            assert args[:5] == (x.data_ptr(), x_next.data_ptr(), net.in_pitch, net.x_off, net.sc_off)
            assert args[6:11] == (4, nz.data_ptr(), 2, 3, 256)
            assert args[11:] == (OBJECTIVES[objective], *head, 1, rederive, *tail, 0)
            assert chain.x0.data_ptr() == net.sc_slice(x_next).data_ptr()
        else:
            assert name == "lgm_sample_step_obj"
            assert args[2:5] == (nz.data_ptr(), x_next.data_ptr(), x0.data_ptr())
            assert args[0] == x.data_ptr() and args[5:9] == (2, 3, 256, 4)
            assert args[9:] == (OBJECTIVES[objective], *head, 1, rederive, *tail, 0)
        assert chain.x is x_next and chain.x_next is x
    # no noise where the step adds none: t == 0 of the ancestral chain, eta == 0 and the last pair of DDIM
    for step in (lambda ch, nz: sampler.p_sample_step(ch, 0, nz), lambda ch, nz: sampler.ddim_step(ch, 999, 979, nz, 0.0),
                 lambda ch, nz: sampler.ddim_step(ch, 19, -1, nz, 1.0)):
        chain = sampler._Chain(gd, shape, torch.randn(shape))
        recorder.calls.clear()
        step(chain, torch.randn(shape))
        (name, args), = recorder.calls
        assert args[7 if self_condition else 2] is None
