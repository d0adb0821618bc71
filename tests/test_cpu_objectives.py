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
