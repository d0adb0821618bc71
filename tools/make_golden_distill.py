"""Generate tests/golden/diffusion_distill.npz: a progressive-distillation step (Salimans & Ho 2022, Algorithm 2) around the
REAL reference's ``Unet`` / ``GaussianDiffusion`` on CPU - two frozen-teacher DDIM steps through the reference's own
``model_predictions(clip_x_start=True, rederive_pred_noise=True)``, the target in the student's objective, the reference's
weighted MSE and ALL student parameter gradients by autograd through the reference's ``Unet``.

TEST INFRASTRUCTURE ONLY, like tools/make_golden_lowres.py, whose stubs (oracle.make_golden.install_stubs), pinned thread
count and ``--check`` mode it shares: it runs where the reference checkout is available and nowhere else.
Usage:  python tools/make_golden_distill.py [--check]

Recipe: the small UNet of diffusion_unet_small.npz (dim 16, 16 x 16, data seed 101), teacher = oracle.unet_init(seed=1),
student = oracle.unet_init(seed=2) (the weights are their seeds: both files rebuild them), T = 1000, N = 4, B = 4 with
i = (0, 1, 2, 3) - every level of the student's grid, the last one with t'' = -1.  Two cases: teacher pred_v -> student pred_v,
teacher pred_noise -> student pred_x0.  Stored per case: z_t, z_t', the float32 torch target, a float64 evaluation of the same
modules (target, loss), the loss, every student gradient (whole up to 512 elements, else norm + a 128-element strided
sample) and the all-parameter gradient norm.  The tool asserts that x~ fed through one step of the reference's DDIM algebra
(``predict_noise_from_start`` and the loop body's update) reproduces the two teacher steps.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
OUT = os.path.join(ROOT, "tests", "golden", "diffusion_distill.npz")

WHOLE, SAMPLE = 512, 128          # gradients up to WHOLE elements are stored whole, larger ones as norm + SAMPLE elements:
                                  # every one of the 283 tensors is in the file, which stays under the committed-file limit

CASES = (("pred_v", "pred_v"), ("pred_noise", "pred_x0"))       # (teacher objective, student objective)
T, N, LEVELS = 1000, 4, (0, 1, 2, 3)
TEACHER_SEED, STUDENT_SEED = 1, 2


def grids(T, N):
    G2 = torch.linspace(-1, T - 1, 2 * N + 1).int().tolist()[::-1]
    return G2[::2], G2


def generate():
    from oracle.make_golden import install_stubs
    install_stubs()                                          # puts the reference on sys.path
    from models.generative.diffusion import ddpm as R
    from oracle import diffusion as O

    torch.set_num_threads(8)
    dim, S, B = 16, 16, len(LEVELS)
    G, G2 = grids(T, N)
    t = torch.tensor([G[i] for i in LEVELS])
    tm = torch.tensor([G2[2 * i + 1] for i in LEVELS])
    tn = torch.tensor([G[i + 1] for i in LEVELS])
    fx = {"dim": dim, "S": S, "B": B, "T": T, "N": N, "data_seed": 101, "teacher_seed": TEACHER_SEED, "student_seed": STUDENT_SEED,
          "i": np.asarray(LEVELS), "t": t.numpy(), "t_mid": tm.numpy(), "t_next": tn.numpy(), "grad_sample": SAMPLE,
          "cases": np.asarray(["%s->%s" % c for c in CASES])}
    g = torch.Generator().manual_seed(101)
    img = torch.rand(B, 3, S, S, generator=g)
    noise = torch.randn(B, 3, S, S, generator=g)

    def network(seed, double=False):
        net = R.Unet(dim=dim, channels=3)
        net.load_state_dict(O.unet_init(dim=dim, channels=3, seed=seed), strict=True)
        if double:
            net.double()
            net.register_forward_pre_hook(lambda m, args: (args[0], args[1].double(), *args[2:]))
        return net

    def distill_target(gd_t, gd_s, o_s, x0, eps):
        """steps 1 - 5 in the dtype of the two diffusions -> (z_t, z_t', target, x~, z_t'')"""
        a, s = gd_s.sqrt_alphas_cumprod, gd_s.sqrt_one_minus_alphas_cumprod
        col = lambda v: v.view(-1, 1, 1, 1)  # noqa: E731
        last = col(tn < 0)
        a_n = torch.where(last, torch.ones_like(col(a[tn.clamp_min(0)])), col(a[tn.clamp_min(0)]))
        s_n = torch.where(last, torch.zeros_like(a_n), col(s[tn.clamp_min(0)]))
        z_t = gd_s.q_sample(x0, t, eps)
        with torch.no_grad():
            e1, x1 = gd_t.model_predictions(z_t, t, None, clip_x_start=True, rederive_pred_noise=True)
            z_m = col(a[tm]) * x1 + col(s[tm]) * e1
            e2, x2 = gd_t.model_predictions(z_m, tm, None, clip_x_start=True, rederive_pred_noise=True)
            z_n = a_n * x2 + s_n * e2
            r = s_n / col(s[t])
            xs = (z_n - r * z_t) / (a_n - r * col(a[t]))
            es = (z_t - col(a[t]) * xs) / col(s[t])
            vs = col(a[t]) * es - col(s[t]) * xs
        return z_t, z_m, {"pred_x0": xs, "pred_noise": es, "pred_v": vs}[o_s], xs, z_n

    for o_t, o_s in CASES:
        pre = f"{o_t}->{o_s}:"
        teacher, student = network(TEACHER_SEED), network(STUDENT_SEED)
        gd_t = R.GaussianDiffusion(teacher, img_size=S, timesteps=T, objective=o_t)
        gd_s = R.GaussianDiffusion(student, img_size=S, timesteps=T, objective=o_s)
        x0 = img * 2 - 1
        z_t, z_m, target, xs, z_n = distill_target(gd_t, gd_s, o_s, x0, noise)
        # one step of the reference's DDIM algebra from z_t with the prediction x~ lands on the two teacher steps
        pn = gd_s.predict_noise_from_start(z_t, t, xs)
        an = torch.where(tn < 0, torch.ones(B), gd_s.alphas_cumprod[tn.clamp_min(0)]).view(-1, 1, 1, 1)
        step = xs * an.sqrt() + (1 - an).sqrt() * pn
        err = float((step - z_n).norm() / z_n.norm())
        assert err < 1e-4, (pre, err)
        fx[pre + "ddim_identity_err"] = np.float64(err)
        fx[pre + "z_t"], fx[pre + "z_mid"], fx[pre + "target"] = z_t.numpy(), z_m.numpy(), target.numpy()
        for p in student.parameters():
            p.grad = None
        out = student(z_t, t)
        loss = (((out - target) ** 2).reshape(B, -1).mean(1) * gd_s.loss_weight[t]).mean()
        loss.backward()
        fx[pre + "loss"] = loss.detach().numpy()
        for n, p in student.named_parameters():
            flat = p.grad.reshape(-1)
            if flat.numel() <= WHOLE:
                fx[pre + "grad:" + n] = p.grad.numpy().copy()
            else:
                fx[pre + "gradnorm:" + n] = np.float64(flat.double().norm().item())
                fx[pre + "gradsample:" + n] = flat[:: flat.numel() // SAMPLE][:SAMPLE].numpy().copy()
        fx[pre + "gradnorm_all"] = np.float64(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in student.parameters())).item())
        # the same modules in float64: the arbiter's side
        t64, s64 = network(TEACHER_SEED, True), network(STUDENT_SEED, True)
        gd_t64 = R.GaussianDiffusion(t64, img_size=S, timesteps=T, objective=o_t).double()
        gd_s64 = R.GaussianDiffusion(s64, img_size=S, timesteps=T, objective=o_s).double()
        z64, _, target64, _, _ = distill_target(gd_t64, gd_s64, o_s, x0.double(), noise.double())
        with torch.no_grad():
            loss64 = (((s64(z64, t) - target64) ** 2).reshape(B, -1).mean(1) * gd_s64.loss_weight[t]).mean()
        fx[pre + "target64"], fx[pre + "loss64"] = target64.numpy(), loss64.numpy()
        print(f"{pre} loss {float(loss.detach()):.6f} (float64 {float(loss64):.6f}), DDIM identity {err:.2e}")
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
