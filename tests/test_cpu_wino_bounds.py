"""CPU: the elementwise check of oracle/winograd.py on every row of the Winograd ledger (tests/test_hip_wino_ledger.py).

First the matrices are proven: the float64 Winograd evaluation equals float64 F.conv2d, conv_transpose2d and conv2d_weight
to 1e-11 of the output scale.  Then every row is evaluated as a float32 Winograd in plain torch - in torch's own einsum
order, and with a strictly sequential sum over the reduction (channels, in phases of 8, for the convolutions; tiles for the
weight gradient) on a slice of the channels - and scored against the direct float64 convolution in units of 2^-24 S_W.  The
worst score per transform (F(2x2), F(4x4)) and kind (conv, weight gradient) must stay under
oracle.winograd.C_WINO_REF_WORST, which is never more than twice the measurement; the kernels get four times the constant.
The mutations a subtly wrong kernel would leave, applied to the float32 evaluation of a row's own inputs, must each score
ABOVE the kernel tolerance on every row named for them: a row that cannot see its mutation has the wrong inputs, not the
wrong tolerance.  The plain and offset rows are named for every mutation that applies to their kind and options.  The two
families whose inputs are mostly zero are named only for what they are built to show (NAMED): one_live_image for the next
image's row read as padding, impulse input gradients for unmirrored taps - impulse forward and impulse weight-gradient rows
check no mutation at all (their part is the float32 reference score, which sets the constants)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import bounds
from oracle import winograd as OW
from test_hip_wino_ledger import LEDGER, families_of, layers_of, problem, row_id, transform_of

_WORST, _WEAKEST, _DONE = {}, {}, {}

# the mutations of the families whose inputs are mostly zero: only the ones those inputs are built to show
NAMED = {
    "one_live_image": {"first row of the next image read as the bottom padding row"},
    "impulse": {"input gradient computed with unmirrored taps"},
}


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("geom", [(2, 8, 8, 5, 3), (1, 6, 10, 3, 4), (3, 4, 4, 2, 2)])
def test_float64_winograd_is_the_convolution(m, geom):
    """maps that are no multiples of the tile included: the matrices, the tiling and the mirrored taps"""
    B, H, W, Cin, Cout = geom
    t = {k: v.double() for k, v in OW.make_inputs(geom, "offset", seed=5).items()}
    y = F.conv2d(t["x"], t["w"], padding=1)
    assert float((OW.conv(t["x"], t["w"], m) - y).abs().max()) < 1e-11 * float(y.abs().max())
    gx = F.conv_transpose2d(t["gy"], t["w"], padding=1)
    assert float((OW.conv(t["gy"], OW.mirrored(t["w"]), m) - gx).abs().max()) < 1e-11 * float(gx.abs().max())
    gw = torch.nn.grad.conv2d_weight(t["x"], (Cout, Cin, 3, 3), t["gy"], padding=1)
    assert float((OW.wgrad(t["gy"], t["x"], m) - gw).abs().max()) < 1e-11 * float(gw.abs().max())
    # the sequential orders are the same sums
    assert float((OW.conv(t["x"], t["w"], m, sequential=True) - y).abs().max()) < 1e-11 * float(y.abs().max())
    assert float((OW.wgrad(t["gy"], t["x"], m, sequential=True) - gw).abs().max()) < 1e-11 * float(gw.abs().max())
    # S_W bounds the result and is at least the direct scale
    S = OW.conv(t["x"].abs(), t["w"].abs(), m, absolute=True)
    assert bool((S >= F.conv2d(t["x"].abs(), t["w"].abs(), padding=1) * (1 - 1e-12)).all())


def _problems(row):
    """(tag, Problem, planes, multi) of everything the row's GPU run scores"""
    o = row["opts"]
    if row["entry"] == "wino_bwd":
        return [(f"{k} {fam}", problem(row, fam, kind=k), k == "wgrad", k == "yx" and bool(o.get("multi")))
                for fam in families_of(row) for k in ("yx", "wgrad")]
    if row["entry"] == "wgradn":
        return [(f"layer {k} {'x'.join(map(str, g))}", pr, True, False) for k, (g, pr) in enumerate(layers_of(row))]
    return [(fam, problem(row, fam), bool(o.get("split", True)), bool(o.get("multi"))) for fam in families_of(row)]


def _evaluate(pr, planes, multi):
    """{order: score}, {mutation: score} of one Problem"""
    key = (pr.kind, pr.m, pr.geom, pr.family, pr.bias, pr.res, pr.beta, pr.seed, planes, multi)
    if key in _DONE:
        return _DONE[key]
    got = pr.eval32()
    nsel, csel = pr.slice_channels()
    sc = {"torch": pr.score(got), "sequential": pr.score(pr.eval32(sequential=True, nsel=nsel, csel=csel), nsel, csel)}
    if pr.kind == "wgrad":
        sc["bias gradient"] = bounds.forward_error_units(pr.eval32_bias(), pr.ref_b, pr.S_b)
        muts = {k: pr.score(v) for k, v in pr.mutations(got, planes=planes).items()}
        # (the bias gradient is bounded by bounds.tolerance(n) of sum |gy|: its score is put on the scale of the row's S_W
        # tolerance, so that "above the tolerance" means the same for every mutation of the row)
        muts["one channel of the fused bias gradient never written"] = \
            bounds.forward_error_units(pr.bias_mutation(pr.eval32_bias()), pr.ref_b, pr.S_b) / bounds.tolerance(pr.n_bias) * pr.tolerance()
    else:
        muts = {k: pr.score(v) for k, v in pr.mutations(got, multi_image=multi, planes=planes).items()}
    if pr.family in NAMED:
        muts = {k: v for k, v in muts.items() if k in NAMED[pr.family]}
    _DONE[key] = (sc, muts)
    return _DONE[key]


def _collect(row, verbose=False):
    """evaluate one row, keep the worst reference scores and the weakest mutations; -> the mutations under the kernel tolerance"""
    m = transform_of(row)
    missed = []
    for tag, pr, planes, multi in _problems(row):
        sc, muts = _evaluate(pr, planes, multi)
        tol = pr.tolerance()
        if verbose:
            print(f"[wino bounds] {row_id(row)} [{tag}]: float32 torch order {sc['torch']:.3f}, sequential {sc['sequential']:.3f} "
                  f"(constant {OW.C_WINO_REF_WORST[(m, pr.ckind)]:g}, kernel tolerance {tol:g})")
        w = _WORST.setdefault((m, pr.ckind), {"torch": (0.0, None), "sequential": (0.0, None)})
        for order in ("torch", "sequential"):
            if sc[order] > w[order][0]:
                w[order] = (sc[order], f"{row_id(row)} [{tag}]")
        for mut, score in muts.items():
            if verbose:
                print(f"[wino bounds]     {mut}: {score:.3g} units")
            if (m, pr.ckind, mut) not in _WEAKEST or score < _WEAKEST[(m, pr.ckind, mut)][0]:
                _WEAKEST[(m, pr.ckind, mut)] = (score, f"{row_id(row)} [{tag}]")
            if not score > tol:
                missed.append((tag, mut, score))
    return missed


@pytest.mark.parametrize("row", LEDGER, ids=row_id)
def test_float32_reference_passes_and_every_mutation_fails(row):
    m = transform_of(row)
    missed = _collect(row, verbose=True)
    for tag, pr, planes, multi in _problems(row):
        sc, muts = _evaluate(pr, planes, multi)
        for order in ("torch", "sequential"):
            assert sc[order] <= OW.C_WINO_REF_WORST[(m, pr.ckind)], (row_id(row), tag, order, sc[order])
        if "bias gradient" in sc:
            assert sc["bias gradient"] < bounds.C_REF_WORST
        if pr.kind == "yx" and pr.family in ("plain", "offset", "impulse"):
            assert "input gradient computed with unmirrored taps" in muts
    assert missed == [], f"mutations the bound does not catch at {row_id(row)}: the row's inputs are wrong, not the bound"


def test_measured_constants_match_the_reference():
    """C_WINO_REF_WORST in oracle/winograd.py is the worst float32 reference score above, rounded up, and never more than twice
    the measurement.  The weakest mutation is printed for the record kept next to the constants."""
    for row in LEDGER:
        _collect(row)
    assert set(_WORST) == set(OW.C_WINO_REF_WORST)
    for key, w in sorted(_WORST.items()):
        worst = max(w["torch"][0], w["sequential"][0])
        print(f"[wino bounds] F({key[0]}x{key[0]}) {key[1]}: worst float32 reference {w['torch'][0]:.3f} in torch's order at "
              f"{w['torch'][1]}, {w['sequential'][0]:.3f} sequential at {w['sequential'][1]}; constant {OW.C_WINO_REF_WORST[key]:g}")
        assert worst <= OW.C_WINO_REF_WORST[key] <= 2.0 * worst, key
        assert OW.tolerance(*key) == 4.0 * OW.C_WINO_REF_WORST[key]
    for key, (score, where) in sorted(_WEAKEST.items(), key=lambda kv: kv[1][0])[:6]:
        print(f"[wino bounds] weakest mutations: {score:.1f} units, F({key[0]}x{key[0]}) {key[1]}: {key[2]} at {where}")
    weakest = min(_WEAKEST.items(), key=lambda kv: kv[1][0] / OW.tolerance(kv[0][0], kv[0][1]))
    assert weakest[1][0] > OW.tolerance(weakest[0][0], weakest[0][1])
    seen = {k[2] for k in _WEAKEST}
    assert seen >= {"one tap dropped at one border pixel", "last output row of one tile replaced by the neighbouring tile's",
                    "one transform-domain point of one tile left out of one phase", "one split-K plane left out of one element",
                    "one slab left out of one element", "one channel's bias omitted", "residual applied twice to one element",
                    "beta = 1 accumulate applied twice to one element", "input gradient computed with unmirrored taps",
                    "first row of the next image read as the bottom padding row",
                    "one coefficient of the output transform doubled on one output row of one tile"}
