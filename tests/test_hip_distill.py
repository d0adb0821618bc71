"""GPU: progressive distillation of the DDPM sampler (``GaussianDiffusion.distill_from``; Salimans & Ho 2022, Algorithm 2; an
extension of the reference).

  * ``lgm_distill_half_step`` / ``lgm_distill_target`` against the float64 restatement of tests/distill_ref.py, per element under
    the derived bound (k + 2) u M / den, all 3 x 3 objective pairs, clip on and off, lane padding, sentinels, both access forms;
  * target, loss and ALL student gradients against the reference's own network (tests/golden/diffusion_distill.npz,
    tools/make_golden_distill.py), 1e-4 relative, the float64 distances on record;
  * graph replay bit for bit against eager launches (plain, accumulating, class-conditional), a model without a teacher against
    one that never had one, a tiny end-to-end round, train.py for two rounds.

Measured distances go through the ``parity`` recorder (committed record: profiles/r19_distill_parity.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distill_ref as DR

pytestmark = pytest.mark.gpu
RTOL = 1e-4
U = DR.U
SENTINEL = 7.0
OBJ = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.shape != b.shape and a.numel() == b.numel():
        a = a.reshape(b.shape)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_distill.npz")))


# ----------------------------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------------------------
def _diffusion(T):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    return GaussianDiffusion(Unet(dim=16), img_size=8, timesteps=T)


def _guarded(shape, dev):
    """a buffer of ``shape`` with 64 sentinel floats in front of it and behind it (16-byte aligned inside)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 128,), SENTINEL, device=dev)
    return flat, flat[64:64 + n].view(shape)


def _nhwc(x, pitch, off, dev, fill=SENTINEL):
    B, C, H, W = x.shape
    buf = torch.full((B, H, W, pitch), fill, device=dev)
    buf[..., off:off + C] = x.permute(0, 2, 3, 1).to(dev)
    return buf


@pytest.mark.parametrize("T,N", [(1000, 4), (1000, 256), (8, 4)])
@pytest.mark.parametrize("shape", [(4, 3, 8, 8), (3, 1, 4, 4)], ids=["4x3x8x8", "3x1x4x4"])
def test_kernels_against_the_float64_restatement(dev, parity, shape, T, N):
    """Per element |kernel - float64| <= (k + 2) u mag: k = distill_ref.ROUNDINGS (the roundings on the longest path, counted in
    the kernel's order with one per table coefficient), mag the expression with magnitudes for operands - it carries the 1 / den
    of the sample's row (M / den).  Levels i = 0, N - 1 (t'' = -1) and interior ones; every objective pair; clip on and off."""
    from lgm_hip import ops
    from lgm_hip.distill import distill_plan
    B, C, H, W = shape
    Cp = (C + 3) // 4 * 4
    gd = _diffusion(T)
    plan = distill_plan(gd, N)
    table = plan.float().to(dev).contiguous()
    G, G2 = DR.grids(T, N)
    idx = [0, N - 1, N // 2, 1][:B]
    t = torch.tensor([G[i] for i in idx])
    row = plan[t].numpy()
    assert np.isfinite(row).all() and row[1, 15] == -1
    g = torch.Generator().manual_seed(T + N + C)
    z_t = torch.randn(shape, generator=g) * 1.2
    o1, o2 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    td = t.to(dev)
    xin, out1, out2 = _nhwc(z_t, Cp, 0, dev), _nhwc(o1, Cp, 0, dev), _nhwc(o2, Cp, 0, dev)
    xin_wide = _nhwc(z_t, 2 * Cp, C, dev)                # the x slice behind another one: the one-lane-per-thread form
    worst = {}
    for ot in range(3):
        for clip in (True, False):
            mid_flat, xmid = _guarded((B, H, W, Cp), dev)
            t_mid = torch.full((B,), -7, dtype=torch.long, device=dev)
            ops.distill_half_step(xin, 0, out1, td, table, ot, clip, xmid, 0, t_mid, C)
            assert ops.lib()._dll.lgm_last_kernel().decode() == "distill_half_step_kernel"
            assert t_mid.tolist() == [G2[2 * i + 1] for i in idx], "t_mid is exact"
            got = xmid.cpu()
            assert bool((mid_flat[:64] == SENTINEL).all()) and bool((mid_flat[-64:] == SENTINEL).all())
            assert bool((got[..., C:] == 0).all()), "padding lanes are zero"
            z_mid = got[..., :C].permute(0, 3, 1, 2).contiguous()
            want, mag, hit = DR.half_step(z_t.double().numpy(), o1.double().numpy(), row, ot, clip)
            if clip and ot != 1:
                assert hit.any() and not hit.all(), "clipping acts on some elements and not on others"
            k = DR.ROUNDINGS["half"]
            err = np.abs(z_mid.double().numpy() - want)
            assert float((err - (k + 2) * U * mag).max()) <= 0, (ot, clip, float((err / mag).max() / U))
            worst["half"] = max(worst.get("half", 0.0), float((err / np.maximum(mag, 1e-300)).max() / U))
            # the scalar form: same bits, nothing outside the slice and its padding
            wide_flat, xmid_w = _guarded((B, H, W, 2 * Cp), dev)
            ops.distill_half_step(xin_wide, C, out1, td, table, ot, clip, xmid_w, Cp, t_mid, C)
            gw = xmid_w.cpu()
            assert torch.equal(gw[..., Cp:], got) and bool((gw[..., :Cp] == SENTINEL).all())
            assert bool((wide_flat[:64] == SENTINEL).all()) and bool((wide_flat[-64:] == SENTINEL).all())
            for os_ in range(3):
                tg_flat, tg = _guarded((B, H, W, Cp), dev)
                ops.distill_target(xin, 0, xmid, 0, out2, td, table, ot, os_, clip, tg, C)
                assert ops.lib()._dll.lgm_last_kernel().decode() == "distill_target_kernel"
                gt = tg.cpu()
                assert bool((tg_flat[:64] == SENTINEL).all()) and bool((tg_flat[-64:] == SENTINEL).all())
                assert bool((gt[..., C:] == 0).all()), "padding lanes are zero"
                want, mag, xs, hit = DR.target(z_t.double().numpy(), z_mid.double().numpy(), o2.double().numpy(), row, ot, os_, clip)
                if clip and ot != 1:
                    assert hit.any() and not hit.all()
                k = DR.ROUNDINGS[os_]
                err = np.abs(gt[..., :C].permute(0, 3, 1, 2).double().numpy() - want)
                assert float((err - (k + 2) * U * mag).max()) <= 0, (ot, os_, clip, float((err / mag).max() / U), k + 2)
                worst[os_] = max(worst.get(os_, 0.0), float((err / np.maximum(mag, 1e-300)).max() / U))
                tw_flat, tgw = _guarded((B, H, W, Cp + 1), dev)      # an odd target pitch: the scalar form again
                ops.distill_target(xin_wide, C, xmid_w, Cp, out2, td, table, ot, os_, clip, tgw, C)
                assert torch.equal(tgw.cpu()[..., :Cp], gt) and bool((tgw[..., Cp:] == SENTINEL).all())
                assert bool((tw_flat[:64] == SENTINEL).all()) and bool((tw_flat[-64:] == SENTINEL).all())
    for what, w in worst.items():
        parity.record(f"distill kernels {shape} T={T} N={N} {what}: worst error in units of u mag (bound {DR.ROUNDINGS[what] + 2}); "
                      f"smallest den {float(row[:, 14].min()):.3e}", err_over_umag=w, bound=DR.ROUNDINGS[what] + 2)
    # x1 from a pred_x0 teacher with |o| > 1 somewhere: clipping acts there too
    assert bool((o1.abs() > 1).any()) and bool((o1.abs() < 1).any())


# ----------------------------------------------------------------------------------------------------------------------
# parity with the reference's own network (dim 16, 16 x 16, T = 1000, N = 4, B = 4: every level of the student's grid)
# ----------------------------------------------------------------------------------------------------------------------
def _pair(fx, case, dev):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    from oracle import diffusion as OD
    o_t, o_s = case.split("->")
    nets = []
    for seed in (int(fx["teacher_seed"]), int(fx["student_seed"])):
        net = Unet(dim=int(fx["dim"]), channels=3)
        net.load_state_dict(OD.unet_init(dim=int(fx["dim"]), channels=3, seed=seed), strict=True)
        nets.append(net)
    S = int(fx["S"])
    teacher = GaussianDiffusion(nets[0], img_size=S, timesteps=int(fx["T"]), objective=o_t)
    student = GaussianDiffusion(nets[1], img_size=S, timesteps=int(fx["T"]), objective=o_s).to(dev)
    nets[1].prepare_hip(dev)
    student.distill_from(teacher, int(fx["N"]))
    return student


@pytest.mark.parametrize("case", ["pred_v->pred_v", "pred_noise->pred_x0"])
def test_target_loss_and_gradients_match_reference_fixture(fx, dev, parity, case):
    from models.generative.diffusion.ddpm import hip_loss_distill, hip_loss_qsample
    gd = _pair(fx, case, dev)
    net = gd.model
    c = {k[len(case) + 1:]: v for k, v in fx.items() if k.startswith(case + ":")}
    B, S = int(fx["B"]), int(fx["S"])
    g = torch.Generator().manual_seed(int(fx["data_seed"]))
    img = torch.rand(B, 3, S, S, generator=g).to(dev)
    noise = torch.randn(B, 3, S, S, generator=g).to(dev)
    t = torch.as_tensor(fx["t"]).to(dev)
    assert gd._distill.grid[:-1] == fx["t"].tolist()
    q = hip_loss_distill(gd, hip_loss_qsample(gd, img, t, noise, True), None)
    target = q.target[..., :3].permute(0, 3, 1, 2)
    parity.record(f"{case}: target [distances to float64]", hip_vs_ref=rel(target, c["target"]),
                  ref_vs_fp64=rel(c["target"], c["target64"]), hip_vs_fp64=rel(target, c["target64"]))
    parity(f"{case}: distillation target", rel(target, c["target"]), RTOL)
    parity(f"{case}: z_t", rel(q.xt[..., :3].permute(0, 3, 1, 2), c["z_t"]), RTOL)
    net._flat.zero_grad()
    loss = gd.p_losses(img, t, noise, _normalize=True)
    want = float(c["loss"])
    parity.record(f"{case}: loss [distances to float64]", hip_vs_ref=abs(loss.item() - want) / want,
                  ref_vs_fp64=abs(want - float(c["loss64"])) / float(c["loss64"]),
                  hip_vs_fp64=abs(loss.item() - float(c["loss64"])) / float(c["loss64"]))
    parity(f"{case}: loss", abs(loss.item() - want) / want, RTOL)
    loss.backward()
    sd = dict(net.named_parameters())
    worst, worst_n, worst_s, seen, Ks = 0.0, 0.0, 0.0, set(), int(fx["grad_sample"])
    for k in c:
        if k.startswith("grad:"):
            worst = max(worst, rel(sd[k[5:]].grad, c[k]))
            seen.add(k[5:])
        elif k.startswith("gradnorm:"):
            n = k[9:]
            worst_n = max(worst_n, abs(sd[n].grad.double().norm().item() - float(c[k])) / max(float(c[k]), 1e-12))
            flat = sd[n].grad.reshape(-1)
            worst_s = max(worst_s, rel(flat[:: flat.numel() // Ks][:Ks], c["gradsample:" + n]))
            seen.add(n)
    assert seen == set(sd), "ALL student parameters are in the fixture"
    parity(f"{case}: worst parameter gradient (whole tensors)", worst, RTOL)
    parity(f"{case}: worst gradient norm (large tensors)", worst_n, RTOL)
    parity(f"{case}: worst {Ks}-element gradient sample (large tensors)", worst_s, RTOL)
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in net.parameters())).item()
    parity(f"{case}: all-parameter gradient norm", abs(gn - float(c["gradnorm_all"])) / float(c["gradnorm_all"]), RTOL)
    assert all(p.grad is None for p in gd._distill.teacher.parameters()), "no gradient reaches the teacher"
    # eval mode uses the same target
    gd.eval()
    with torch.no_grad():
        assert torch.equal(gd.p_losses(img, t, noise, _normalize=True), loss.detach())
    net._flat.zero_grad()


# ----------------------------------------------------------------------------------------------------------------------
# the graph-replayed step, a model without a teacher, end to end, train.py
# ----------------------------------------------------------------------------------------------------------------------
def _module(dev, **kw):
    from models.generative.diffusion.ddpm import DDPM
    torch.manual_seed(10)
    m = DDPM(**dict(dict(img_size=16, dim=16, lr=1e-3, ema_update_every=2), **kw))
    m.sample_every = 0
    m.to(dev)
    m.prepare_hip(dev)
    m.train()
    return m


@pytest.mark.parametrize("kw,acc", [(dict(), 1), (dict(objective="pred_noise"), 2), (dict(num_classes=3), 1)],
                         ids=["plain_step", "accumulate2", "class_conditional"])
def test_graph_replayed_distillation_step_equals_eager_steps(dev, kw, acc):
    """Four steps through ``make_fast_step``: losses, parameters after Adam, the EMA shadow and the Adam state of graph replay and
    eager launches are the same bits; every drawn t lies on the student's grid and two replays draw different ones."""
    a, b = _module(dev, distill_steps=4, **kw), _module(dev, distill_steps=4, **kw)
    oa, ob = a.configure_optimizers(), b.configure_optimizers()
    fa, fb = a.make_fast_step(oa, 1, True, accumulate=acc), b.make_fast_step(ob, 1, False, accumulate=acc)
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(8, 3, 16, 16, generator=g).to(dev) for _ in range(4)]
    y = (torch.arange(8) % 3).to(dev)
    losses, drawn = {}, []
    for name, fast in (("graph", fa), ("eager", fb)):
        torch.manual_seed(77)
        losses[name] = []
        for i, x in enumerate(xs):
            losses[name].append(fast.step((x.clone(), y), i).detach().clone().reshape(()))
            if name == "graph":
                drawn.append(fast.graphed.t.clone())
    assert fa.mode.startswith("hipGraph") and fb.mode == "eager"
    for la, lb in zip(losses["graph"], losses["eager"]):
        assert torch.isfinite(la) and torch.equal(la, lb), (float(la), float(lb))
    grid = set(a.ema.online_model._distill.grid[:-1])
    assert all(set(t.tolist()) <= grid for t in drawn) and len({tuple(t.tolist()) for t in drawn}) > 1
    na, nb = a.ema.online_model.model, b.ema.online_model.model
    assert torch.equal(na._flat.data, nb._flat.data)
    assert torch.equal(a.ema.ema_model.model._flat.data, b.ema.ema_model.model._flat.data)
    ta, w0 = a.ema.online_model._distill.teacher, _module(dev, **kw).ema.online_model.model
    assert torch.equal(ta._flat.data, w0._flat.data), "the teacher is frozen at the weights the round started from"
    assert not torch.equal(na._flat.data, w0._flat.data), "the student trains"
    for pa, pb in zip(oa.state_dict()["state"].values(), ob.state_dict()["state"].values()):
        for k in pb:
            assert torch.equal(torch.as_tensor(pa[k]), torch.as_tensor(pb[k])), k
    # the next round is captured anew: the step object notices the new teacher
    a.halve()
    b.halve()
    torch.manual_seed(5)
    la = fa.step((xs[0].clone(), y), 4).detach().clone()
    torch.manual_seed(5)
    lb = fb.step((xs[0].clone(), y), 4).detach().clone()
    assert torch.equal(la.reshape(()), lb.reshape(())) and set(fa.graphed.t.tolist()) <= {999, 499}


def test_a_model_without_a_teacher_is_the_parent_behaviour(dev):
    """Same seed: a model whose teacher was detached and one that never had a teacher draw the same t and noise and return the
    same loss bits, in the captured step and in eager ``forward``; the eager forward draws t ~ randint(0, T), noise and nothing more."""
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    x = torch.rand(8, 3, 16, 16, device=dev)
    y = torch.zeros(8, dtype=torch.long, device=dev)
    got = {}
    for name in ("never", "detached"):
        m = _module(dev)
        if name == "detached":
            m.start_distillation(4)                  # (the student starts at the weights it has: nothing moves)
            m.ema.online_model.distill_from(None)
        fast = m.make_fast_step(m.configure_optimizers(), 1, True)
        torch.manual_seed(123)
        loss = fast.step((x.clone(), y), 0).detach().clone()
        assert fast.mode.startswith("hipGraph") and fast.graphed.distill_sig is None
        got[name] = (fast.graphed.t.clone(), fast.graphed.noise.clone(), loss, m.ema.online_model.model._flat.data.clone())
    for a, b in zip(got["never"], got["detached"]):
        assert torch.equal(a, b)
    assert int(got["never"][0].max()) < 1000 and len(set(got["never"][0].tolist()) - {999, 749, 499, 249}) > 0
    torch.manual_seed(3)
    net = Unet(dim=16)
    gd = GaussianDiffusion(net, img_size=16).to(dev)
    net.prepare_hip(dev)
    torch.manual_seed(55)
    with torch.no_grad():
        gd(x)
    after = torch.rand(4, device=dev)
    torch.manual_seed(55)
    torch.randint(0, 1000, (8,), device=dev)
    torch.randn_like(x)
    assert torch.equal(after, torch.rand(4, device=dev))


E2E_TEACHER_STEPS, E2E_STEPS, E2E_LR = 150, 30, 2e-4


def test_a_tiny_round_moves_the_student_towards_the_teachers_longer_chain(dev, parity, monkeypatch):
    """dim 16, 8 x 8, T = 1000, N = 2, batch 8, E2E_STEPS optimizer steps from a student initialised at the teacher: the
    distillation loss falls, and from one initial noise the student's 2-step ``ddim_sample`` is nearer (mean squared distance) to
    the teacher's 4-step ``ddim_sample`` than the teacher's own 2-step ``ddim_sample`` is.

    The teacher is a TRAINED one, as distillation presumes: the module first trains plainly for E2E_TEACHER_STEPS steps on the
    batch (lr 1e-3), then its online weights become the round's teacher and the student trains E2E_STEPS steps at E2E_LR.
    Fixed once from a float32 CPU run of the same recipe with autograd over the oracle's UNet (other draws): four teacher seeds
    times two round seeds give a teacher 2-step distance of 0.0069 - 0.0072 and a student distance of 0.0020 - 0.0025 (0.0030
    and 0.0045 from a teacher trained 400 steps).  Measured on the MI355X, this seed: loss 0.00663 -> 0.00274, student 0.002451
    against the teacher's 0.007170.  From an UNTRAINED teacher the same round moves the student away (0.0130 against 0.0053
    measured on the MI355X, 0.0124 - 0.0129 on the CPU, at no step count up to 300 or learning rate down to 5e-5 otherwise):
    under pred_v ``loss_weight[999]`` is 3e-7, so the first of the two student steps is held by nothing but the weights it
    shares with the second, and the second is trained on q_sample inputs an untrained teacher's chain never
    visits.  The 30 steps and the inequality are the issue's."""
    from lgm_hip import sampler
    from models.generative.diffusion.ddpm import GaussianDiffusion
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")          # three diffusions over two networks, one chain each: eager launches
    m = _module(dev, img_size=8)
    on = m.ema.online_model
    g = torch.Generator().manual_seed(21)
    data = torch.rand(8, 3, 8, 8, generator=g).to(dev)
    y = torch.zeros(8, dtype=torch.long, device=dev)
    fast = m.make_fast_step(m.configure_optimizers(), 1, True)
    torch.manual_seed(30)
    plain = [float(fast.step((data.clone(), y), i)) for i in range(E2E_TEACHER_STEPS)]
    assert np.isfinite(plain).all()
    print(f"[distill e2e] teacher: plain loss first ten {np.mean(plain[:10]):.4f} last ten {np.mean(plain[-10:]):.4f}")
    m.start_distillation(2, source="online")
    m.hparams["lr"] = E2E_LR
    fast = m.make_fast_step(m.configure_optimizers(), 1, True)          # a new round: new moments, the step captured anew
    torch.manual_seed(31)
    losses = [float(fast.step((data.clone(), y), i)) for i in range(E2E_STEPS)]
    assert fast.mode.startswith("hipGraph") and fast.graphed.distill_sig is not None
    first, last = float(np.mean(losses[:6])), float(np.mean(losses[-6:]))
    print(f"[distill e2e] loss first six {first:.5f} last six {last:.5f}")
    shape = (8, 3, 8, 8)
    init = torch.randn(shape, generator=torch.Generator().manual_seed(41)).to(dev)
    teacher = lambda n: GaussianDiffusion(on._distill.teacher, img_size=8, sampling_timesteps=n).to(dev)      # noqa: E731
    run = lambda gd: sampler.ddim_sample(gd, shape, init_noise=init.clone()).clone()  # noqa: E731
    t4, t2, s2 = run(teacher(4)), run(teacher(2)), run(on)
    d_student, d_teacher = float(((s2 - t4) ** 2).mean()), float(((t2 - t4) ** 2).mean())
    parity.record(f"distill end to end ({E2E_TEACHER_STEPS} teacher steps, {E2E_STEPS} student steps): mean squared distance to "
                  f"the teacher's 4-step sample", student_2_steps=d_student, teacher_2_steps=d_teacher, loss_first=first,
                  loss_last=last)
    print(f"[distill e2e] to the teacher's 4-step sample: student 2-step {d_student:.6f}, teacher 2-step {d_teacher:.6f}")
    assert on.sampling_timesteps == 2 and torch.isfinite(s2).all()
    assert last < first, (first, last)
    assert d_student < d_teacher, (d_student, d_teacher)


def test_train_entry_runs_two_distillation_rounds(tmp_path):
    """train.py's main() on configs/diffusion/ddpm_distill.json at a reduced size (8 x 8, dim 16, distill_steps 4): two rounds of
    three steps; the checkpoint holds the second round's teacher and step count."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightning-generative-models_amd")
    cfg = json.load(open(os.path.join(pkg, "configs", "diffusion", "ddpm_distill.json")))
    assert cfg["model"]["args"]["distill_steps"] == 128
    cfg["model"]["args"].update(img_size=8, dim=16, distill_steps=4)
    cfg["dataset"].update(img_size=8, batch_size=8)
    path = tmp_path / "ddpm_distill_small.json"
    path.write_text(json.dumps(cfg))
    exp = "pytest_gpu_diffusion_ddpm_distill"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); import train; m = train.main(sys.argv[2:]); "
            "print('STEPS', m.ema.online_model.distill_steps, m.global_step, m.trainer.fast.mode); "
            "print('TRAIN_LOSS', float(m.logged['train_loss']))")
    cmd = [sys.executable, "-c", code, pkg, "--config_path", str(path), "--distill_rounds", "2", "--distill_round_steps", "3",
           "--experiment_name", exp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("STEPS", "TRAIN_LOSS"))}
    assert lines["STEPS"].startswith("STEPS 2 6 hipGraph replay"), lines
    assert np.isfinite(float(lines["TRAIN_LOSS"].split()[1]))
    assert "[distill] round 1/2: 8 -> 4" in r.stdout and "[distill] round 2/2: 4 -> 2" in r.stdout
    ck = os.path.join(pkg, "experiments", cfg["model"]["name"], exp, "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 6 and sd["hyper_parameters"]["distill_steps"] == 2
    assert int(sd["state_dict"]["ema.online_model.distill_steps"]) == 2
    assert "ema.online_model.distill_teacher.init_conv.weight" in sd["state_dict"]
    for v in sd["state_dict"].values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
