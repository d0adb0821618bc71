"""No GPU: the dropout mask's definition (tests/dropout_ref.py) against Philox4x32-10's known answers and against the statistics
a mask must have, the host's threshold / scale, constructor validation, and that dropout adds no state to the model."""
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

import dropout_ref as R

KEY = 0x9E3779B91234ABCD
SHAPES = [((2, 16, 64), 0), ((3, 35, 64), 7), ((2, 64, 128), 18)]      # ((B, HW, C), layer)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w) for w in R.philox4x32_10(ctr, key))
    assert got == want, [hex(g) for g in got]


def test_counter_and_key_layout():
    """element n of layer L, pass P under key K: word (n & 3) of Philox(counter (q lo, q hi, L, P), key (K lo, K hi)), q = n >> 2"""
    w = R.words((2, 3, 8), KEY, 5, 1)
    flat = w.reshape(-1)
    for n in (0, 1, 7, 13, 47):
        q = n >> 2
        one = R.philox4x32_10((q, 0, 5, 1), (KEY & 0xFFFFFFFF, KEY >> 32))
        assert int(flat[n]) == int(one[n & 3])


@pytest.mark.parametrize("p,thr", [(0.0, 0), (0.1, 429496729), (0.5, 2147483648), (0.999, 4290672328)])
def test_threshold_and_scale(p, thr):
    from lgm_hip import ops
    t, s = ops.dropout_operands(p)
    assert t == thr == min(2 ** 32 - 1, math.floor(p * 2.0 ** 32)) == R.operands(p)[0]
    assert s == float(np.float32(1.0 / (1.0 - p))) == float(R.operands(p)[1])
    assert ops.dropout_operands(1.0 - 2.0 ** -40)[0] == 2 ** 32 - 1          # the clamp


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, True, False, "0.1", None, float("nan"), float("inf")])
def test_constructors_refuse_what_is_no_probability(bad):
    from models.generative.diffusion.ddpm import DDPM, Unet
    with pytest.raises(ValueError) as e:
        Unet(dim=8, dim_mults=(1, 2), dropout=bad)
    assert repr(bad) in str(e.value)
    with pytest.raises(ValueError) as e:
        DDPM(img_size=16, dim=16, dropout=bad)
    assert repr(bad) in str(e.value)


def test_dropout_adds_no_state():
    from models.generative.diffusion.ddpm import DDPM, GaussianDiffusion, Unet
    a, b = Unet(dim=8, dim_mults=(1, 2)), Unet(dim=8, dim_mults=(1, 2), dropout=0.3)
    assert b.dropout == 0.3 and a.dropout == 0.0
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    ga, gb = (GaussianDiffusion(n, img_size=16) for n in (a, b))
    assert list(ga.state_dict()) == list(gb.state_dict())
    assert inspect.signature(Unet.__init__).parameters["dropout"].default == 0.0
    assert inspect.signature(DDPM.__init__).parameters["dropout"].default == 0.0
    m = DDPM(img_size=16, dim=16, dropout=0.1)
    assert m.hparams["dropout"] == 0.1 and m.ema.online_model.model.dropout == 0.1
    assert m.ema.ema_model.model.dropout == 0.0, "the EMA shadow never drops"
    assert list(m.state_dict()) == list(DDPM(img_size=16, dim=16).state_dict())
    assert gb.draw_dropout_key("cpu") is not None and ga.draw_dropout_key("cpu") is None
    gb.eval()
    assert gb.draw_dropout_key("cpu") is None, "evaluation mode draws no key"


def test_config_is_ddpm_plus_dropout():
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lightning-generative-models_amd", "configs",
                        "diffusion")
    base = json.load(open(os.path.join(here, "ddpm.json")))
    drop = json.load(open(os.path.join(here, "ddpm_dropout.json")))
    assert drop["model"]["args"].pop("dropout") == 0.1
    assert drop == base
    from utils.loader import load_config, load_model
    cfg = load_config(os.path.join(here, "ddpm_dropout.json"))
    assert load_model(cfg["model"]).ema.online_model.model.dropout == 0.1


def test_c_abi_of_the_new_entry_points():
    from lgm_hip import _lib
    protos = _lib.parse_header()
    for name, n in (("lgm_dropout_fwd", 11), ("lgm_dropout_bwd", 11), ("lgm_gn_fwd_drop", 30), ("lgm_gn_bwd_drop", 38)):
        assert name in protos and len(protos[name][1]) == n, (name, len(protos.get(name, (0, []))[1]))
    L = _lib.lib()
    assert L.lgm_abi_version() == 8
    with pytest.raises(_lib.LgmArgumentError, match="dropout"):      # rejected on the host: no launch
        L.lgm_dropout_fwd(None, 8, 1, 1, 8, None, 0, 0, 0, 1.0, None)
    with pytest.raises(_lib.LgmArgumentError, match="dropout operands"):
        L.lgm_dropout_fwd(64, 8, 1, 1, 8, 64, 0, 0, 2 ** 32, 1.0, None)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape,layer", SHAPES)
def test_keep_rate(shape, layer, p):
    k = R.keep(shape, KEY, layer, 0, p)
    n = k.size
    sigma = math.sqrt(p * (1 - p) / n)
    dev = abs(float(k.mean()) - (1 - p)) / sigma
    print(f"keep rate {shape} layer {layer} p {p}: {k.mean():.5f}, {dev:.2f} sigma")
    assert dev < 4.0


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape,layer", SHAPES)
def test_masks_of_layers_passes_and_keys_are_independent(shape, layer, p):
    base = R.keep(shape, KEY, layer, 0, p)
    a = p * p + (1 - p) * (1 - p)
    sigma = math.sqrt(a * (1 - a) / base.size)
    for what, other in (("layer", R.keep(shape, KEY, layer + 1, 0, p)), ("pass", R.keep(shape, KEY, layer, 1, p)),
                        ("key", R.keep(shape, KEY ^ 1, layer, 0, p)), ("key, high half", R.keep(shape, KEY ^ (1 << 32), layer, 0, p))):
        dev = abs(float((base == other).mean()) - a) / sigma
        print(f"agreement across {what} {shape} p {p}: {dev:.2f} sigma")
        assert dev < 4.0, what


def test_apply_scales_kept_and_zeroes_dropped():
    x = np.random.default_rng(0).standard_normal((2, 16, 64)).astype(np.float32)
    y = R.apply(x, KEY, 3, 0, 0.25)
    k = R.keep(x.shape, KEY, 3, 0, 0.25)
    assert np.array_equal(y[k], x[k] * np.float32(1.0 / 0.75)) and not np.signbit(y[~k]).any() and (y[~k] == 0).all()
    assert torch.equal(torch.as_tensor(R.apply(x, KEY, 3, 0, 0.0)), torch.as_tensor(x))
