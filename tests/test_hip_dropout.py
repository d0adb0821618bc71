"""GPU: dropout without a mask tensor (csrc/lgm_philox.h) against its numpy restatement (tests/dropout_ref.py).

  1. the stand-alone kernels: kept / dropped elements and the kept values to the bit, NaN guard lanes untouched;
  2. the fused GroupNorm forward (tensor input and split-K planes) = the plain launch of the same plan followed by the host's
     where(keep, fl32(y * scale), 0), to the bit, saved statistics included - every plan of the norm ledger's GroupNorm rows,
     the two-pass plans (stand-alone kernel behind them) too;
  3. the fused GroupNorm backward with gy as one tensor = the plain backward on the host-premasked gy, to the bit;
  4. the fused GroupNorm backward with gy as planes against float64 (oracle/norm.py) under the ledger's own bounds;
  5. (not needed: no comparison of 2 or 3 had to be loosened - the select between the product v * scale and +0 keeps the
     compiler from contracting that product into the sums behind it);
  6. the whole network's loss and parameter gradients against oracle.diffusion with the reference mask on every ``block1``;
  7. the training step: graph replay = eager launches to the bit, one key per (micro-)step, the loss moves;
  8. dropout off - p = 0, evaluation mode, samplers, the likelihood - gives the bits and the draws of a model without it."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dropout_ref as R
from oracle import norm as N
from test_hip_norm_ledger import LEDGER, Buffers, problem, row_id

pytestmark = pytest.mark.gpu
RTOL = 1e-4
KEY = 0x9E3779B91234ABCD
_DIST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


def key_tensor(dev, key=KEY):
    return torch.tensor([key - 2 ** 64 if key >= 2 ** 63 else key], dtype=torch.int64, device=dev)


def drop_args(keyt, layer, pass_, p):
    from lgm_hip import ops
    thr, scale = ops.dropout_operands(p)
    assert (thr, np.float32(scale)) == R.operands(p)
    return (keyt.data_ptr(), layer, pass_, thr, scale)


def host_mask(t, shape, layer, pass_, p, key=KEY):
    """where(keep, fl32(t * scale), +0) on the host, t a float32 tensor of ``shape`` = (B, HW, C) elements"""
    return torch.from_numpy(R.apply(t.detach().cpu().numpy().reshape(shape), key, layer, pass_, p))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a).reshape(-1), bits(b).reshape(-1)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pitch(t):
    return 0 if t is None else t.stride(0)


# ---- 1. the stand-alone kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("shape,layer,p,sliced", [((2, 16, 64), 0, 0.1, False), ((3, 35, 64), 7, 0.5, True), ((2, 64, 128), 18, 0.25, False)])
def test_standalone_kernels_against_the_reference_mask(dev, which, shape, layer, p, sliced):
    from lgm_hip import ops
    B, HW, C = shape
    x = torch.randn(B, HW, C, generator=torch.Generator().manual_seed(layer))
    x[0, 0, :4] = torch.tensor([float("inf"), -0.0, 2.0 ** -100, -3.0])
    lo, hi = (8, 4) if sliced else (0, 0)                 # a channel slice of a wider buffer between NaN guard lanes
    buf = torch.full((B, HW, 1, lo + C + hi), float("nan"), device=dev)
    view = buf[..., lo:lo + C]
    view.copy_(x.reshape(B, HW, 1, C))
    keyt = key_tensor(dev)
    (ops.dropout_fwd if which == "fwd" else ops.dropout_bwd)(view, drop_args(keyt, layer, 1, p))
    torch.cuda.synchronize()
    want = host_mask(x, shape, layer, 1, p)
    got = view.cpu().reshape(shape)
    keep = torch.from_numpy(R.keep(shape, KEY, layer, 1, p))
    assert torch.equal(got != 0, keep & (x != 0)), "kept / dropped elements"
    assert same_bits(got, want), "kept values are fl32(x * scale), dropped ones +0"
    assert bool(torch.isnan(buf[..., :lo]).all()) and bool(torch.isnan(buf[..., lo + C:]).all()), "guard lanes"
    assert 0 < int(keep.sum()) < keep.numel()


# ---- 2 / 3 / 4. the GroupNorm launches -----------------------------------------------------------------------------------------
GN_ROWS = [r for r in LEDGER if r["kind"] == "gn"]
ONE_PASS = sorted({r["plan"][1:] for r in GN_ROWS if r["plan"][2] > 0})
PLANE_ROWS = [r for r in LEDGER if r["kind"] == "planes" and r["opts"]["splits"] in (3, 16)]      # 16: whole rounds and a tail


def test_every_one_pass_pair_is_covered():
    from test_hip_norm_ledger import registry_names
    pairs = {tuple(int(v) for v in n[len("gn_fused_fwd_kernel<"):-1].split(", ")) for n in registry_names()
             if n.startswith("gn_fused_fwd_kernel<")}
    assert set(ONE_PASS) == pairs and len(pairs) == 8
    assert {r["plan"][2] for r in PLANE_ROWS} == {1, 2, 8} and len(PLANE_ROWS) == 6


def _forward(row, pr, dev, drop):
    """One forward launch of the row (``drop``: the dropout operands or None) -> dict of device outputs, guards intact"""
    from lgm_hip import ops
    L, st, o, t = ops.lib(), ops.stream(), row["opts"], pr.t
    B, C, H, W, G = row["geom"]
    P = H * W
    bf = Buffers(dev)
    gamma, beta = bf.flat(t["gamma"]), bf.flat(t["beta"])
    ss = bf.pitched(t["ss"], lo=4, hi=8) if o["film"] else None
    res = bf.pitched(t["res"].reshape(B * P, C), lo=0, hi=4) if o["res"] else None
    y = bf.pitched(shape=(B * P, C))
    mean, rstd, A, Bc = bf.flat(n=B * G), bf.flat(n=B * G), bf.flat(n=B * C), bf.flat(n=B * C)
    tail = (B, P, C, G, N.EPS, gamma.data_ptr(), beta.data_ptr(), _ptr(ss), _pitch(ss), int(o["act"]), _ptr(res), _pitch(res),
            y.data_ptr(), _pitch(y), mean.data_ptr(), rstd.data_ptr(), A.data_ptr(), Bc.data_ptr())
    got = {"mean": mean, "rstd": rstd, "A": A, "Bc": Bc, "y": y}
    if row["kind"] == "planes":
        xp = bf.flat(t["xp"])
        cbias = bf.flat(t["cbias"]) if o["cbias"] else None
        x = got["xw"] = bf.pitched(shape=(B * P, C), lo=4, hi=8)
        head = (xp.data_ptr(), B * P * C, o["splits"], _ptr(cbias), x.data_ptr(), _pitch(x))
        if drop is None:
            L.lgm_gn_fwd_planes(*head, *tail, st)
        else:
            L.lgm_gn_fwd_drop(*head, *tail, *drop, st)
    else:
        x = bf.pitched(t["x"].reshape(B * P, C), lo=4, hi=8)
        if drop is None:
            L.lgm_gn_fwd(x.data_ptr(), _pitch(x), *tail, st)
        else:
            L.lgm_gn_fwd_drop(None, 0, 0, None, x.data_ptr(), _pitch(x), *tail, *drop, st)
    torch.cuda.synchronize()
    assert bf.intact(), "a NaN guard lane around an operand or an output was written"
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("row", GN_ROWS + PLANE_ROWS, ids=row_id)
def test_fused_forward_equals_plain_launch_then_host_mask(dev, row):
    B, C, H, W, G = row["geom"]
    layer, p = LEDGER.index(row) % 19, 0.25
    pr = problem(row)
    keyt = key_tensor(dev)
    plain = _forward(row, pr, dev, None)
    fused = _forward(row, pr, dev, drop_args(keyt, layer, 0, p))
    want = host_mask(plain["y"], (B, H * W, C), layer, 0, p)
    assert same_bits(fused["y"], want), "y: where(keep, fl32(y * scale), 0) of the plain launch"
    for k in plain:
        if k != "y":
            assert same_bits(fused[k], plain[k]), k
    kept = float((fused["y"] != 0).float().mean())
    assert 0.6 < kept < 0.9, kept


def _backward(row, pr, dev, drop, gy32=None, planes=None):
    """One backward launch: gy as a tensor (``gy32`` [B, P, C]) or as the row's planes.  ``drop`` None: the plain entry points."""
    from lgm_hip import ops
    L, st, o, t = ops.lib(), ops.stream(), row["opts"], pr.t
    B, C, H, W, G = row["geom"]
    P, film, act = H * W, o["film"], int(o["act"])
    mode = "plain" if o["mode"] == "add" else o["mode"]      # (no residual gradient rides beside a dropout launch)
    bf = Buffers(dev)
    gamma, beta = bf.flat(t["gamma"]), bf.flat(t["beta"])
    ss = bf.pitched(t["ss"], lo=4, hi=8) if film else None
    x = bf.pitched(t["x"].reshape(B * P, C), lo=4, hi=8)
    gy = bf.pitched(gy32.reshape(B * P, C), lo=8, hi=4) if planes is None else None
    gyp = bf.flat(planes) if planes is not None else None
    sm, sr, sA, sB = (bf.flat(pr.sv[k]) for k in ("mean", "rstd", "A", "Bc"))
    acc = mode == "acc"
    gx = bf.pitched(t["gx0"].reshape(B * P, C) if acc else None, shape=(B * P, C))
    gg, gb = bf.flat(t["gg0"] if acc else None, n=C), bf.flat(t["gb0"] if acc else None, n=C)
    gss = bf.pitched(t["gss0"] if acc else None, shape=(B, 2 * C), lo=4, hi=4) if film else None
    ws = torch.empty(5 * B * C, device=dev)
    deferred = mode == "deferred"
    rws = bf.flat(n=B * 2 * C) if deferred else None
    desc = (ctypes.c_int64 * 8)() if deferred else None
    dp = None if desc is None else ctypes.addressof(desc)
    b1 = 1.0 if acc else 0.0
    mid = (B, P, C, G, gamma.data_ptr(), beta.data_ptr(), _ptr(ss), _pitch(ss), act, sm.data_ptr(), sr.data_ptr(), sA.data_ptr(),
           sB.data_ptr(), gx.data_ptr(), _pitch(gx), int(acc), gg.data_ptr(), gb.data_ptr(), b1, _ptr(gss), _pitch(gss), b1, ws.data_ptr())
    xa = (x.data_ptr(), _pitch(x))
    if drop is not None:
        L.lgm_gn_bwd_drop(*xa, _ptr(gy), _pitch(gy), _ptr(gyp), B * P * C if planes is not None else 0,
                          planes.shape[0] if planes is not None else 0, *mid, _ptr(rws), dp, *drop, st)
    elif planes is not None:
        L.lgm_gn_bwd_planes(*xa, gyp.data_ptr(), B * P * C, planes.shape[0], *mid, _ptr(rws), dp, st)
    elif deferred:
        L.lgm_gn_bwd_deferred(*xa, gy.data_ptr(), _pitch(gy), *mid, rws.data_ptr(), dp, st)
    else:
        L.lgm_gn_bwd(*xa, gy.data_ptr(), _pitch(gy), *mid, st)
    if desc is not None:
        assert (desc[6] > 0) == (row["plan"][2] > 0), "only the one-pass kernel defers its gamma / beta rows"
        if desc[6] > 0:
            ops.wgrad_reduce_batch([tuple(desc)], dev)
    torch.cuda.synchronize()
    assert bf.intact(), "a NaN guard lane around an operand or an output was written"
    out = {"gx": gx.cpu(), "ggamma": gg.cpu(), "gbeta": gb.cpu()}
    if film:
        out["gss"] = gss.cpu()
    return out, mode


@pytest.mark.parametrize("row", GN_ROWS, ids=row_id)
def test_fused_backward_equals_plain_backward_of_premasked_gy(dev, row):
    B, C, H, W, G = row["geom"]
    layer, p = LEDGER.index(row) % 19, 0.25
    pr = problem(row)
    keyt = key_tensor(dev)
    gy = pr.t["gy"]
    plain, _ = _backward(row, pr, dev, None, gy32=host_mask(gy, (B, H * W, C), layer, 0, p))
    fused, _ = _backward(row, pr, dev, drop_args(keyt, layer, 0, p), gy32=gy)
    for k in plain:
        assert same_bits(fused[k], plain[k]), k


@pytest.mark.parametrize("row", PLANE_ROWS, ids=row_id)
def test_fused_backward_from_planes_against_float64(dev, row, parity):
    B, C, H, W, G = row["geom"]
    o = row["opts"]
    layer, p = LEDGER.index(row) % 19, 0.25
    pr = problem(row)
    keyt = key_tensor(dev)
    got, mode = _backward(row, pr, dev, drop_args(keyt, layer, 0, p), planes=pr.t["gyp"])
    keep = torch.from_numpy(R.keep((B, H * W, C), KEY, layer, 0, p)).double() * float(R.operands(p)[1])
    gyp = pr.t["gyp"].double()
    d, sv64 = N.to(pr.t, torch.float64), N.to(pr.sv, torch.float64)
    ref = N.gn_backward(d, sv64, G, o["film"], o["act"], mode, gy=gyp.sum(0) * keep)
    S = N.gn_backward(d, sv64, G, o["film"], o["act"], mode, gy=gyp.sum(0) * keep, scales=True, Sgy=gyp.abs().sum(0) * keep)
    for k in got:
        g = got[k].reshape(ref[k].shape)
        score, rel = N.forward_error_units(g, ref[k], S[k]), N.rel(g, ref[k])
        parity(f"gn_fused_bwd_drop {row_id(row).split('|', 2)[2]} {k} [units of 2^-24 S]", score, N.tolerance())
        assert score < N.tolerance_blocked() and rel < RTOL, (k, score, rel)


# ---- 6. the whole network ----------------------------------------------------------------------------------------------------
def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _block_names(n_stages=4):
    names = []
    for i in range(n_stages):
        names += [f"downs.{i}.0", f"downs.{i}.1"]
    names += ["mid_block1", "mid_block2"]
    for i in range(n_stages):
        names += [f"ups.{i}.0", f"ups.{i}.1"]
    return names + ["final_res_block"]


class _MaskedOracle:
    """oracle.diffusion with ``block`` wrapped: the output of every ``*.block1`` is multiplied by the reference mask of its
    layer under ``pass_`` (set by the caller around each network pass)."""

    def __init__(self, monkeypatch, p, key=KEY):
        from oracle import diffusion as OD
        self.OD, self.p, self.key, self.pass_ = OD, p, key, 0
        self.layers = {n + ".block1": k for k, n in enumerate(_block_names())}
        orig = OD.block

        def block(P, pre, x, scale_shift=None, groups=8):
            out = orig(P, pre, x, scale_shift, groups)
            if pre in self.layers:
                B, C, H, W = out.shape
                keep = R.keep((B, H * W, C), self.key, self.layers[pre], self.pass_, self.p)
                m = torch.from_numpy(keep).reshape(B, H, W, C).permute(0, 3, 1, 2).to(out.dtype) * float(R.operands(self.p)[1])
                out = out * m
            return out
        monkeypatch.setattr(OD, "block", block)


def _record(name, values):
    _DIST[name] = values
    path = os.environ.get("LGM_DROPOUT_PARITY")      # the committed copy is profiles/r17_dropout_parity.json
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(_DIST, fh, indent=1, sort_keys=True)


def _grad_distances(net, P):
    sd = dict(net.named_parameters())
    return {k: rel(sd[k].grad, P[k].grad) for k in P}


def test_network_loss_and_gradients_match_the_masked_oracle(dev, monkeypatch, parity):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    mo = _MaskedOracle(monkeypatch, 0.25)
    OD = mo.OD
    dim, S, B = 16, 16, 2
    P = {k: v.clone().requires_grad_(True) for k, v in OD.unet_init(dim=dim, channels=3, seed=3).items()}
    assert len(_block_names()) == 19
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    noise = torch.randn(B, 3, S, S, generator=g)
    t = torch.tensor([37, 812])
    net = Unet(dim=dim, channels=3, dropout=0.25)
    net.load_state_dict({k: v.detach() for k, v in P.items()}, strict=True)
    gd = GaussianDiffusion(net, img_size=S, timesteps=1000).to(dev)
    net.prepare_hip(dev)
    gd.train()
    keyt = key_tensor(dev)
    loss = gd.p_losses(x0.to(dev), t.to(dev), noise.to(dev), _dropout_key=keyt)
    loss.backward()
    ref = OD.p_losses(P, OD.diffusion_buffers(1000), x0, t, noise, dim=dim)
    ref.backward()
    dist = _grad_distances(net, P)
    dl = abs(loss.item() - ref.item()) / ref.item()
    _record("plain network, B = 2 at 16 x 16, p = 0.25", {"loss": dl, "worst gradient": max(dist.values()), "gradients": dist})
    parity("loss", dl, RTOL)
    parity(f"worst parameter gradient ({len(dist)} tensors)", max(dist.values()), RTOL)
    # the unmasked oracle would miss the bound by an order of magnitude: it is met because of the mask, not in spite of it
    mo.p = 0.0
    far = OD.p_losses({k: v.detach() for k, v in P.items()}, OD.diffusion_buffers(1000), x0, t, noise, dim=dim)
    assert abs(far.item() - ref.item()) / ref.item() > 10 * RTOL


def test_self_conditioned_network_matches_the_masked_oracle(dev, monkeypatch, parity):
    """pass 1 of the mask in the estimate, pass 0 in the trained pass"""
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    mo = _MaskedOracle(monkeypatch, 0.25)
    OD = mo.OD
    dim, S, B = 16, 16, 2
    P = OD.unet_init(dim=dim, channels=3, seed=4)
    P["init_conv.weight"] = torch.randn(dim, 6, 7, 7, generator=torch.Generator().manual_seed(9)) * (6 * 49) ** -0.5
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    g = torch.Generator().manual_seed(6)
    x0 = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    noise = torch.randn(B, 3, S, S, generator=g)
    t = torch.tensor([503, 90])
    net = Unet(dim=dim, channels=3, self_condition=True, dropout=0.25)
    net.load_state_dict({k: v.detach() for k, v in P.items()}, strict=True)
    gd = GaussianDiffusion(net, img_size=S, timesteps=1000).to(dev)
    net.prepare_hip(dev)
    gd.train()
    loss = gd.p_losses(x0.to(dev), t.to(dev), noise.to(dev), _self_cond=True, _dropout_key=key_tensor(dev))
    loss.backward()
    bufs = OD.diffusion_buffers(1000)
    xt = OD.q_sample(bufs, x0, t, noise)
    with torch.no_grad():
        mo.pass_ = 1
        v = OD.unet_forward({k: p.detach() for k, p in P.items()}, torch.cat((torch.zeros_like(xt), xt), dim=1), t, dim)
        est = OD._ext(bufs["sqrt_alphas_cumprod"], t, 4) * xt - OD._ext(bufs["sqrt_one_minus_alphas_cumprod"], t, 4) * v
    mo.pass_ = 0
    out = OD.unet_forward(P, torch.cat((est, xt), dim=1), t, dim)
    per = torch.nn.functional.mse_loss(out, OD.predict_v(bufs, x0, t, noise), reduction="none").reshape(B, -1).mean(1)
    ref = (per * bufs["loss_weight"].gather(-1, t)).mean()
    ref.backward()
    dist = _grad_distances(net, P)
    dl = abs(loss.item() - ref.item()) / ref.item()
    _record("self-conditioned network, B = 2 at 16 x 16, p = 0.25", {"loss": dl, "worst gradient": max(dist.values()), "gradients": dist})
    parity("loss", dl, RTOL)
    parity(f"worst parameter gradient ({len(dist)} tensors)", max(dist.values()), RTOL)


# ---- 7. the training step -------------------------------------------------------------------------------------------------------
def _module(dev, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(img_size=16, dim=16, lr=1e-3, ema_update_every=2, **kw)
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


def _run_steps(dev, use_graph, n, accumulate=1, **kw):
    m = _module(dev, **kw)
    opt = m.configure_optimizers()
    fast = m.make_fast_step(opt, 1, use_graph, accumulate=accumulate)
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(4, 3, 16, 16, generator=g).to(dev) for _ in range(n)]
    torch.manual_seed(77)                                      # the device generator: same draws in every run
    losses, keys = [], []
    for i, x in enumerate(xs):
        losses.append(fast.step((x.clone(), None), i).detach().clone().reshape(()))
        k = m.ema.online_model.__dict__.get("dropout_key")
        keys.append(None if k is None else int(k.item()))
    fast.flush()
    torch.cuda.synchronize()
    return m, fast, losses, keys, torch.cuda.get_rng_state(dev)


@pytest.mark.parametrize("accumulate", [1, 2])
def test_graph_replayed_step_equals_eager_steps(dev, accumulate):
    n = 3 if accumulate == 1 else 4
    a, fa, la, ka, ra = _run_steps(dev, True, n, accumulate, dropout=0.25)
    b, fb, lb, kb, rb = _run_steps(dev, False, n, accumulate, dropout=0.25)
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    for x, y in zip(la, lb):
        assert torch.isfinite(x) and torch.equal(x, y), (float(x), float(y))
    assert ka == kb and None not in ka and len(set(ka)) == n, "one key per (micro-)step, the same in both runs"
    assert torch.equal(a.ema.online_model.model._flat.data, b.ema.online_model.model._flat.data)
    assert torch.equal(a.ema.ema_model.model._flat.data, b.ema.ema_model.model._flat.data)
    if accumulate == 1:
        c, fc, lc, kc, rc = _run_steps(dev, True, n)            # the same seed without dropout
        assert kc == [None] * n and "dropout_key" not in c.ema.online_model.__dict__
        assert all(not torch.equal(x, z) for x, z in zip(la, lc)), "the loss moves under dropout"
        assert not torch.equal(ra, rc), "the key draw advances the generator"


# ---- 8. dropout off ------------------------------------------------------------------------------------------------------------
def _nets(dev, S=16, **gdkw):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    P = OD.unet_init(dim=16, channels=3, seed=11)
    out = []
    for kw in (dict(), dict(dropout=0.0), dict(dropout=0.3)):
        net = Unet(dim=16, channels=3, **kw)
        net.load_state_dict(P, strict=True)
        gd = GaussianDiffusion(net, img_size=S, timesteps=1000, **gdkw).to(dev)
        net.prepare_hip(dev)
        out.append(gd)
    return out


def test_dropout_off_gives_the_bits_of_a_model_without_it(dev):
    plain, zero, drop = _nets(dev, sampling_timesteps=3)
    g = torch.Generator().manual_seed(2)
    img = torch.rand(2, 3, 16, 16, generator=g).to(dev)
    x0, noise, t = img * 2 - 1, torch.randn(2, 3, 16, 16, generator=g).to(dev), torch.tensor([10, 700], device=dev)
    keyt = key_tensor(dev)
    for gd in (plain, zero, drop):
        gd.train()
    with torch.no_grad():
        want = plain.p_losses(x0, t, noise)
        assert torch.equal(zero.p_losses(x0, t, noise, _dropout_key=keyt), want), "dropout = 0.0, training mode, a key handed in"
        dropped = drop.p_losses(x0, t, noise, _dropout_key=keyt)
        assert torch.isfinite(dropped) and not torch.equal(dropped, want), "dropout = 0.3 in training mode drops"
        drop.eval()
        assert torch.equal(drop.p_losses(x0, t, noise, _dropout_key=keyt), want), "dropout = 0.3 in evaluation mode"
        assert torch.equal(drop.p_losses(x0, t, noise), want)
        drop.train()
        # the network as a module, the samplers and the likelihood never drop, whatever the mode
        assert torch.equal(drop.model(x0, t), plain.model(x0, t))
        outs = []
        for gd in (plain, drop):
            torch.manual_seed(5)
            outs.append(gd.sample(batch_size=2))
        assert torch.equal(outs[0], outs[1]), "sample() of a training-mode model with dropout 0.3"
        vs = []
        for gd in (plain, drop):
            torch.manual_seed(6)
            vs.append(gd.vlb_terms(img, timesteps=[999, 500, 0]))
        assert torch.equal(vs[0].vb, vs[1].vb) and torch.equal(vs[0].prior_bpd, vs[1].prior_bpd), "vlb_terms"


def test_a_step_without_dropout_draws_what_it_drew(dev):
    """the generator state after a ``dropout=0`` step = the state after the same step on a model built without the argument"""
    for use_graph in (True, False):
        a = _run_steps(dev, use_graph, 2)
        b = _run_steps(dev, use_graph, 2, dropout=0.0)
        assert torch.equal(a[4], b[4]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
        assert b[3] == [None, None]
