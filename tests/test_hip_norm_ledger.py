"""The ledger of the norm kernels (csrc/norm.hip): every name the library can note there is RUN at a small shape that
routes to it, `lgm_last_kernel()` and the host planner's answer (`lgm_gn_plan`) are compared with the row, and every output -
the saved mean / rstd / coefA / coefB included - is compared with float64 ELEMENTWISE in units of 2^-24 * S (oracle/norm.py;
the tolerance is four times what tests/test_cpu_norm_bounds.py measures on the float32 CPU reference, and a second, narrower
bound is four times what it measures in torch's own blocked order) as well as by the ratio of norms the per-op tests use.  Operands and outputs sit in pitched buffers between NaN guard lanes that must stay
untouched, and the reduced gradients of two runs must be bit-equal.

A GroupNorm row runs the forward AND the backward pass of its shape: both follow the same plan (cb channels per block, nt
threads, nv 16-byte values per thread; nv = 0: the two-pass kernels), so a row carries two names.  gn_apply_kernel,
gn_bwd_apply_kernel and gn_bwd_affine_kernel have one instantiation each and always follow one of the named kernels: the
same row's outputs check them.

The planner (gn_plan in norm.hip): cb = Cg * ceil(32 / Cg) channels (at most C); while B * C / cb < 256 blocks and cb is more
than one group, cb is halved (never below 8 channels, always whole groups and whole quads).  nt = 1024 where HW * cb >= 16384,
else 256; the one-pass kernel runs with the first nt of (that, 256, 128, 64) for which tq = cb / 4 divides nt, ppb = nt / tq
divides HW and (nt, nv = HW / ppb) is an instantiated pair; else two passes at the first nt.

The completeness tests need no GPU."""
import ctypes
import re

import pytest
import torch

from oracle import norm as N

RTOL = 1e-4
FAMILIES = ("gn_fused_fwd_kernel", "gn_fused_bwd_kernel", "gn_stats_kernel", "gn_bwd_reduce_kernel", "gn_coef_from_stats_kernel",
            "rmsnorm_fwd_kernel", "rmsnorm_bwd_kernel")


def _gn_names(plan):
    cb, nt, nv = plan
    if nv:
        return (f"gn_fused_fwd_kernel<{nt}, {nv}>", f"gn_fused_bwd_kernel<{nt}, {nv}>")
    return (f"gn_stats_kernel<{nt}>", f"gn_bwd_reduce_kernel<{nt}>")


def GN(geom, plan, why, family="plain", film=False, act=False, res=False, mode="plain"):
    return {"kind": "gn", "geom": tuple(geom), "plan": tuple(plan), "names": _gn_names(plan), "why": why,
            "opts": dict(family=family, film=film, act=act, res=res, mode=mode)}


def PL(geom, plan, splits, cbias, why, film=False, act=False, res=False, mode="plain"):
    return {"kind": "planes", "geom": tuple(geom), "plan": tuple(plan), "names": _gn_names(plan), "why": why,
            "opts": dict(splits=splits, cbias=cbias, film=film, act=act, res=res, mode=mode)}


def ST(geom, parts, cbias, offset, why, film=False, act=False, res=False):
    return {"kind": "stats", "geom": tuple(geom), "plan": None, "names": ("gn_coef_from_stats_kernel",), "why": why,
            "opts": dict(parts=parts, cbias=cbias, offset=offset, film=film, act=act, res=res)}


def RMS(geom, why, res=False, mode="plain", zero_pixel=False):
    q = max(1, geom[1] // 256)
    return {"kind": "rms", "geom": tuple(geom), "plan": None, "names": (f"rmsnorm_fwd_kernel<{q}>", f"rmsnorm_bwd_kernel<{q}>"),
            "why": why, "opts": dict(res=res, mode=mode, zero_pixel=zero_pixel)}


# GroupNorm geometry = (B, C, H, W, G); plan = (cb, nt, nv)
LEDGER = [
    # ---- one-pass kernels, 1024 threads: HW * cb >= 16384, nv = HW * cb / 4096
    GN((1, 256, 16, 32, 8), (32, 1024, 4), "Cg = 32 = cb (one group: no narrowing); 512 * 32 = 16384 -> 1024 threads, ppb = 128, nv = 4",
       film=True, act=True, res=True),
    GN((1, 256, 32, 32, 8), (32, 1024, 8), "Cg = 32 = cb; 1024 * 32 = 32768 -> ppb = 128, nv = 8", family="offset", act=True, mode="add"),
    # ---- 256 / 128 / 64 threads, blocks 32 channels wide: B * C / 32 = 256 blocks already (or Cg = 32)
    GN((128, 64, 4, 4, 8), (32, 128, 1), "256 blocks: cb = 32, tq = 8; 16 pixels: ppb = 32 does not divide -> 128 threads, ppb = 16, nv = 1",
       film=True, act=True, mode="deferred"),
    GN((128, 64, 8, 8, 8), (32, 256, 2), "256 blocks: cb = 32; 64 pixels, ppb = 32, nv = 2", film=True, act=True, res=True, mode="acc"),
    GN((2, 64, 16, 16, 2), (32, 256, 8), "Cg = 32 = cb; 256 * 32 = 8192 < 16384 -> 256 threads, ppb = 32, nv = 8", family="small"),
    GN((128, 64, 2, 4, 8), (32, 64, 1), "cb = 32, 8 pixels: ppb = 32, 16 do not divide -> 64 threads, ppb = 8, nv = 1", res=True, mode="acc"),
    GN((128, 64, 4, 8, 8), (32, 256, 1), "cb = 32, 32 pixels = ppb, nv = 1", film=True, act=True, res=True, mode="add"),
    GN((2, 64, 8, 16, 2), (32, 256, 4), "Cg = 32 = cb; 128 pixels, ppb = 32, nv = 4", family="offset", film=True, act=True),
    # ---- the same plans narrowed to one group: B * C / cb = 4 < 256 -> cb = 32 -> 16 -> 8 = Cg, tq = 2
    GN((2, 64, 8, 8, 8), (8, 128, 1), "cb = 8: 64 pixels, ppb = 128 does not divide -> 128 threads, ppb = 64, nv = 1", family="offset",
       film=True, res=True),
    GN((2, 64, 16, 16, 8), (8, 256, 2), "cb = 8: 256 pixels, ppb = 128, nv = 2", act=True, res=True, mode="deferred"),
    GN((1, 64, 4, 8, 8), (8, 64, 1), "cb = 8: 32 pixels: ppb = 128, 64 do not divide -> 64 threads, ppb = 32, nv = 1", film=True, act=True,
       mode="add"),
    GN((2, 64, 8, 16, 8), (8, 256, 1), "cb = 8: 128 pixels = ppb, nv = 1", film=True, mode="deferred"),
    GN((2, 64, 16, 32, 8), (8, 256, 4), "cb = 8: 512 pixels, ppb = 128, nv = 4", act=True, mode="acc"),
    GN((2, 64, 32, 32, 8), (8, 256, 8), "cb = 8: 1024 * 8 = 8192 < 16384 -> 256 threads, ppb = 128, nv = 8", film=True, act=True, res=True),
    # ---- two-pass kernels
    GN((2, 64, 4, 4, 8), (8, 256, 0), "cb = 8, 16 pixels: no ppb of 128 / 64 / 32 divides them -> two passes, 256 threads", family="small",
       film=True, act=True, res=True),
    GN((1, 64, 64, 64, 4), (16, 1024, 0), "Cg = 16: cb = 32 -> 16; 4096 * 16 = 65536 -> nv = 16 at 1024 threads, 64 at 256: no pair",
       film=True, act=True, res=True, mode="acc"),
    GN((2, 72, 8, 8, 6), (36, 256, 0), "Cg = 12 -> cb = 36 (18 is no whole group): tq = 9 divides no thread count; 252 of 256 threads active",
       film=True, act=True, mode="deferred"),
    GN((2, 96, 8, 8, 4), (24, 256, 0), "Cg = 24 -> cb = 48 -> 24: tq = 6 divides no thread count", family="offset", act=True, res=True,
       mode="add"),
    GN((1, 72, 24, 24, 6), (36, 1024, 0), "cb = 36, 576 * 36 = 20736 >= 16384 -> two passes at 1024 threads, 1017 active", film=True),
    # ---- group widths
    GN((2, 32, 8, 8, 32), (8, 128, 1), "Cg = 1: cb = 32 -> 16 -> 8 (never below 8): 8 groups per block, one quad spans 4 groups", film=True,
       act=True, res=True),
    GN((128, 64, 4, 4, 32), (32, 128, 1), "Cg = 2, 256 blocks: cb = 32 holds 16 groups, one quad spans 2", act=True, mode="acc"),
    GN((2, 32, 16, 16, 8), (8, 256, 2), "Cg = 4: cb = 32 -> 8, two groups per block, one quad per group", film=True, res=True, mode="deferred"),
    GN((2, 128, 8, 8, 2), (64, 256, 4), "Cg = 64 = cb: tq = 16, ppb = 16, nv = 4", film=True, act=True),
    GN((2, 256, 4, 4, 2), (128, 256, 2), "Cg = 128 = cb: tq = 32, ppb = 8, nv = 2", act=True, res=True, mode="add"),
    GN((2, 256, 4, 4, 1), (256, 256, 4), "G = 1: cb = C = 256, tq = 64, ppb = 4, nv = 4; J = nt / cb = 1 part per channel", film=True, act=True,
       res=True, mode="acc"),
    # ---- maps that are not square: 35 and 15 pixels divide by no ppb
    GN((3, 64, 5, 7, 8), (8, 256, 0), "cb = 8: ppb = 128 / 64 / 32 -> two passes, 35 of 128 pixel lanes busy", film=True, act=True, res=True),
    GN((2, 128, 3, 5, 8), (16, 256, 0), "Cg = 16: cb = 32 -> 16, tq = 4: ppb = 64 / 32 / 16 do not divide 15", family="offset"),
] + [
    # ---- split-K planes summed by the one-pass kernels: PR = 8 planes per round at NV = 1, 4 at NV = 2, 2 at NV >= 4, then a tail
    PL(geom, plan, splits, cbias, f"{why}; {splits} planes", film=fl, act=ac, res=rs, mode=md)
    for geom, plan, why, fl, ac, rs in [
        ((2, 64, 8, 8, 8), (8, 128, 1), "NV = 1: rounds of 8", True, True, False),
        ((2, 64, 16, 16, 8), (8, 256, 2), "NV = 2: rounds of 4", False, True, True),
        ((2, 64, 16, 16, 2), (32, 256, 8), "NV = 8: rounds of 2", True, False, True),
    ]
    for splits, cbias, md in [(1, True, "plain"), (2, False, "acc"), (3, True, "deferred"), (9, False, "plain"), (16, True, "acc"),
                              (17, False, "deferred")]
] + [
    # ---- statistics from float32 rows of (sum, sum of squares): the float64 combine, and the block that measures x itself
    ST((2, 64, 8, 8, 8), 1, True, False, "Cg = 8: J = 8 row lanes, one row", film=True, act=True),
    ST((2, 64, 8, 8, 8), 3, False, True, "Cg = 8, 3 rows; mean square / variance = 3600 > 1e3: the block measures x", act=True, res=True),
    ST((2, 64, 8, 8, 8), 16, True, True, "Cg = 8, 16 rows = 2 per lane; offset input with bias", film=True, res=True),
    ST((2, 64, 8, 8, 1), 1, False, True, "Cg = 64: J = 1, every thread one channel; offset input", film=True, act=True, res=True),
    ST((2, 64, 8, 8, 1), 3, True, False, "Cg = 64, 3 rows in sequence", act=True),
    ST((2, 64, 8, 8, 1), 16, False, False, "Cg = 64, 16 rows in sequence", film=True),
] + [
    # ---- RMSNorm: L = min(64, C / 4) lanes per pixel, 256 / L pixels per block pass, Q = C / 256 quads per lane, <= 1024 blocks
    RMS((3, 4, 7, 13), "C = 4: L = 1, 256 pixels per block; 273 pixels = 1 block + 17", res=True),
    RMS((3, 8, 7, 13), "C = 8: L = 2, 128 pixels per block; 273 = 2 blocks + 17", mode="acc"),
    RMS((3, 64, 5, 7), "C = 64: L = 16, 16 pixels per block; 105 = 6 blocks + 9; a zero pixel and one of norm 1e-3", res=True,
        mode="deferred", zero_pixel=True),
    RMS((1, 256, 3, 5), "C = 256: L = 64, Q = 1, 4 pixels per block; 15 = 3 blocks + 3", res=True, mode="acc", zero_pixel=True),
    RMS((1, 512, 3, 5), "C = 512: Q = 2", mode="deferred"),
    RMS((1, 1024, 3, 5), "C = 1024: Q = 4", res=True, zero_pixel=True),
    RMS((5, 256, 29, 29), "4205 pixels = 1052 block passes > the cap of 1024 blocks: the grid-stride loop runs twice in 28 blocks",
        res=True, mode="acc"),
]


def row_id(row):
    o = row["opts"]
    tag = "".join(k[0] for k in ("film", "act", "res") if o.get(k)) or "-"
    extra = {"gn": lambda: f"{o['family']}-{o['mode']}", "planes": lambda: f"s{o['splits']}{'b' if o['cbias'] else ''}-{o['mode']}",
             "stats": lambda: f"p{o['parts']}{'b' if o['cbias'] else ''}{'-offset' if o['offset'] else ''}",
             "rms": lambda: f"{o['mode']}{'-zero' if o['zero_pixel'] else ''}"}[row["kind"]]()
    return f"{row['names'][0]}|{row['kind']}|{'x'.join(map(str, row['geom']))}|{tag}|{extra}"


_PROBLEMS = {}


def problem(row):
    """The row's operands, float64 results and scales, never changed by a test.  One row at a time is kept (the float64
    tensors of a large row take 100 MB): the tests of one row follow each other."""
    key = row_id(row)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()
        o, seed = row["opts"], LEDGER.index(row)
        if row["kind"] == "rms":
            _PROBLEMS[key] = N.RMSProblem(row["geom"], o["res"], o["mode"], o["zero_pixel"], seed)
        elif row["kind"] == "gn":
            _PROBLEMS[key] = N.GNProblem(row["geom"], o["family"], o["film"], o["act"], o["res"], o["mode"], seed)
        elif row["kind"] == "planes":
            _PROBLEMS[key] = N.GNProblem(row["geom"], "plain", o["film"], o["act"], o["res"], o["mode"], seed, kind="planes",
                                         splits=o["splits"], cbias=o["cbias"])
        else:
            _PROBLEMS[key] = N.GNProblem(row["geom"], "plain", o["film"], o["act"], o["res"], "plain", seed, kind="stats",
                                         parts=o["parts"], cbias=o["cbias"], offset=o["offset"])
    return _PROBLEMS[key]


def _dll():
    from lgm_hip import _lib
    D = _lib.lib()._dll
    D.lgm_kernel_name.restype = ctypes.c_char_p
    return D


def registry_names():
    D = _dll()
    return sorted({D.lgm_kernel_name(i).decode() for i in range(D.lgm_kernel_name_count())})


def gn_plan(B, HW, C, G, bwd):
    """(cb, nt, nv) from the library's host planner, None where the shape is not supported"""
    cb, nt, nv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = _dll().lgm_gn_plan(B, HW, C, G, bwd, ctypes.byref(cb), ctypes.byref(nt), ctypes.byref(nv))
    return (cb.value, nt.value, nv.value) if rc == 0 else None


# ---- completeness (no GPU) ------------------------------------------------------------------------------------------------
def test_every_norm_kernel_name_has_a_ledger_row():
    names = [n for n in registry_names() if n.startswith(FAMILIES)]
    keys = {n for r in LEDGER for n in r["names"]}
    assert len(names) >= 20 and {n.split("<")[0] for n in names} == set(FAMILIES)
    assert sorted(set(names) - keys) == [], "names norm.hip can note without a ledger row"
    assert sorted(keys - set(names)) == [], "ledger rows whose name the library can never note"
    assert len({row_id(r) for r in LEDGER}) == len(LEDGER)
    assert all(r["why"] for r in LEDGER)


def test_the_planner_agrees_with_every_row():
    from lgm_hip import _lib
    L = _lib.lib()
    for r in LEDGER:
        if r["plan"] is None:
            continue
        B, C, H, W, G = r["geom"]
        for bwd in (0, 1):
            assert gn_plan(B, H * W, C, G, bwd) == r["plan"], (row_id(r), r["why"])
        if r["kind"] == "planes":
            assert L.lgm_gn_planes_supported(B, H * W, C, G) == 1


def test_every_instantiation_of_the_dispatch_is_reachable():
    """A sweep of the planner over batch sizes, square and rectangular maps and the supported (C, G) pairs returns every
    (nt, nv) pair the launchers switch over (the registry names of the one-pass kernels) and both thread counts of the
    two-pass kernels - an instantiation no shape reaches would be dead code - and never a pair without a kernel."""
    names = registry_names()
    want = {(bwd, int(m.group(2)), int(m.group(3))) for n in names
            for m in [re.fullmatch(r"gn_fused_(fwd|bwd)_kernel<(\d+), (\d+)>", n)] if m
            for bwd in [int(m.group(1) == "bwd")]}
    want |= {(bwd, int(m.group(2)), 0) for n in names for m in [re.fullmatch(r"gn_(stats|bwd_reduce)_kernel<(\d+)>", n)] if m
             for bwd in [int(m.group(1) == "bwd_reduce")]}
    assert len(want) == 20
    seen = set()
    sides = (2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 29, 32, 48, 64)
    for C in (4, 8, 16, 32, 64, 72, 96, 128, 192, 256, 384, 512, 1024):
        for G in (1, 2, 4, 6, 8, 16, 32, 64):
            if gn_plan(1, 4, C, G, 0) is None:
                continue
            for B in (1, 2, 3, 4, 8, 16, 32, 64, 128, 256, 512):
                for i, H in enumerate(sides):
                    for W in sides[i:]:
                        for bwd in (0, 1):
                            cb, nt, nv = gn_plan(B, H * W, C, G, bwd)
                            assert cb % (C // G) == 0 and cb % 4 == 0 and C % cb == 0
                            seen.add((bwd, nt, nv))
    assert seen - want == set(), "the planner returns a pair the launchers have no kernel for"
    assert want - seen == set(), "instantiations no swept shape reaches"


# ---- running one row ---------------------------------------------------------------------------------------------------------
NAN = float("nan")


class Buffers:
    """Device buffers of one row, every one between NaN guards: pitched [R, C] views (pitch C + lo + hi, lo % 4 == 0) and
    flat 16-byte aligned vectors.  Outputs start as NaN: an element the kernel does not write scores inf."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def pitched(self, src=None, shape=None, lo=4, hi=4):
        R, C = shape if src is None else src.shape
        buf = torch.full((R, C + lo + hi), NAN, device=self.dev)
        view = buf[:, lo:lo + C]
        if src is not None:
            view.copy_(src)
        self.all.append((buf, lo, C))
        return view

    def flat(self, src=None, n=None):
        n = n if src is None else src.numel()
        buf = torch.full((n + 64,), NAN, device=self.dev)
        view = buf[32:32 + n]
        if src is not None:
            view.copy_(src.reshape(-1))
        self.all.append((buf, 32, n))
        return view

    def intact(self):
        return all(bool(torch.isnan(b[..., :lo]).all()) and bool(torch.isnan(b[..., lo + n:]).all()) for b, lo, n in self.all)


def _last():
    from lgm_hip import ops
    k = ops.lib()._dll.lgm_last_kernel()
    return k.decode() if k else ""


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pitch(t):
    return 0 if t is None else t.stride(0)


def _check(out, stage, got, ref, S):
    for k in S:
        g = got[k].detach().cpu().reshape(ref[k].shape)
        out["checks"].append({"what": f"{stage} {k}", "score": N.forward_error_units(g, ref[k], S[k]), "rel": N.rel(g, ref[k])})


def _run_gn(row, pr, dev, out):
    from lgm_hip import ops
    L, st, o, t = ops.lib(), ops.stream(), row["opts"], pr.t
    B, C, H, W, G = row["geom"]
    P, kind = H * W, row["kind"]
    film, act, mode = o["film"], int(o["act"]), o.get("mode", "plain")
    bf = Buffers(dev)
    gamma, beta = bf.flat(t["gamma"]), bf.flat(t["beta"])
    ss = bf.pitched(t["ss"], lo=4, hi=8) if film else None
    res = bf.pitched(t["res"].reshape(B * P, C), lo=0, hi=4) if o["res"] else None
    y = bf.pitched(shape=(B * P, C))
    mean, rstd, A, Bc = bf.flat(n=B * G), bf.flat(n=B * G), bf.flat(n=B * C), bf.flat(n=B * C)
    tail = (B, P, C, G, N.EPS, gamma.data_ptr(), beta.data_ptr(), _ptr(ss), _pitch(ss), act, _ptr(res), _pitch(res), y.data_ptr(),
            _pitch(y), mean.data_ptr(), rstd.data_ptr(), A.data_ptr(), Bc.data_ptr(), st)
    cbias = bf.flat(t["cbias"]) if o.get("cbias") else None
    got = {"mean": mean, "rstd": rstd, "A": A, "Bc": Bc, "y": y}
    if kind == "gn":
        x = bf.pitched(t["x"].reshape(B * P, C), lo=4, hi=8)
        L.lgm_gn_fwd(x.data_ptr(), _pitch(x), *tail)
    elif kind == "planes":
        xp = bf.flat(t["xp"])
        x = got["xw"] = bf.pitched(shape=(B * P, C), lo=4, hi=8)          # written by the kernel
        L.lgm_gn_fwd_planes(xp.data_ptr(), B * P * C, o["splits"], _ptr(cbias), x.data_ptr(), _pitch(x), *tail)
    else:
        x = bf.pitched(t["x"].reshape(B * P, C), lo=4, hi=8)
        rows = bf.flat(t["rows"])
        L.lgm_gn_fwd_stats(rows.data_ptr(), o["parts"], _ptr(cbias), x.data_ptr(), _pitch(x), *tail)
    out["names"].append(_last())
    torch.cuda.synchronize()
    _check(out, "forward", got, pr.ref_f, pr.S_f)
    if kind == "stats":
        out["guards"] = bf.intact()
        return
    # ---- backward, from the float64 forward's saved values rounded to float32 (twice: the reduced gradients must be bit-equal)
    if kind == "planes":
        x = bf.pitched(t["x"].reshape(B * P, C), lo=4, hi=8)
        gyp = bf.flat(t["gyp"])
    else:
        gy = bf.pitched(t["gy"].reshape(B * P, C), lo=8, hi=4)
    sm, sr, sA, sB = (bf.flat(pr.sv[k]) for k in ("mean", "rstd", "A", "Bc"))
    acc = mode == "acc"
    runs = []
    for _ in range(2):
        gx = bf.pitched(t["gx0"].reshape(B * P, C) if acc else None, shape=(B * P, C))
        gg, gb = bf.flat(t["gg0"] if acc else None, n=C), bf.flat(t["gb0"] if acc else None, n=C)
        gss = bf.pitched(t["gss0"] if acc else None, shape=(B, 2 * C), lo=4, hi=4) if film else None
        add = bf.pitched(t["add0"].reshape(B * P, C), lo=4, hi=4) if mode == "add" else None
        ws = torch.empty(5 * B * C, device=dev)
        rws = bf.flat(n=B * 2 * C) if mode == "deferred" else None
        desc = (ctypes.c_int64 * 8)() if mode == "deferred" else None
        dp = None if desc is None else ctypes.addressof(desc)
        beta1 = 1.0 if acc else 0.0
        mid = (B, P, C, G, gamma.data_ptr(), beta.data_ptr(), _ptr(ss), _pitch(ss), act, sm.data_ptr(), sr.data_ptr(), sA.data_ptr(),
               sB.data_ptr(), gx.data_ptr(), _pitch(gx), int(acc), gg.data_ptr(), gb.data_ptr(), beta1, _ptr(gss), _pitch(gss), beta1,
               ws.data_ptr())
        if kind == "planes":
            L.lgm_gn_bwd_planes(x.data_ptr(), _pitch(x), gyp.data_ptr(), B * P * C, o["splits"], *mid, _ptr(rws), dp, st)
        elif mode == "deferred":
            L.lgm_gn_bwd_deferred(x.data_ptr(), _pitch(x), gy.data_ptr(), _pitch(gy), *mid, rws.data_ptr(), dp, st)
        elif mode == "add":
            L.lgm_gn_bwd_add(x.data_ptr(), _pitch(x), gy.data_ptr(), _pitch(gy), *mid, None, None, add.data_ptr(), _pitch(add), st)
        else:
            L.lgm_gn_bwd(x.data_ptr(), _pitch(x), gy.data_ptr(), _pitch(gy), *mid, st)
        out["names"].append(_last())
        if desc is not None:
            assert (desc[6] > 0) == (row["plan"][2] > 0), "only the one-pass kernel defers its gamma / beta rows"
            if desc[6] > 0:
                ops.wgrad_reduce_batch([tuple(desc)], dev)
        torch.cuda.synchronize()
        g = {"gx": gx, "ggamma": gg, "gbeta": gb}
        if film:
            g["gss"] = gss
        if add is not None:
            g["add"] = add
        runs.append(g)
    _check(out, "backward", runs[0], pr.ref_b, pr.S_b)
    out["names"] = out["names"][:2] + ([] if out["names"][2] == out["names"][1] else [out["names"][2]])
    out["deterministic"] = all(bool(torch.equal(runs[0][k], runs[1][k])) for k in runs[0])
    out["guards"] = bf.intact()


def _run_rms(row, pr, dev, out):
    from lgm_hip import ops
    L, st, o, t = ops.lib(), ops.stream(), row["opts"], pr.t
    B, C, H, W = row["geom"]
    npix, mode = B * H * W, o["mode"]
    bf = Buffers(dev)
    x, gy, g = bf.pitched(t["x"], lo=4, hi=4), bf.pitched(t["gy"], lo=0, hi=8), bf.flat(t["g"])
    res = bf.pitched(t["res"], lo=8, hi=0) if o["res"] else None
    y = bf.pitched(shape=(npix, C))
    L.lgm_rmsnorm_fwd(x.data_ptr(), _pitch(x), g.data_ptr(), _ptr(res), _pitch(res), y.data_ptr(), _pitch(y), npix, C, st)
    out["names"].append(_last())
    torch.cuda.synchronize()
    _check(out, "forward", {"y": y}, pr.ref_f, pr.S_f)
    if o["zero_pixel"]:          # x = 0: y is the residual to the bit (0 where there is none)
        want = t["res"][1] if o["res"] else torch.zeros(C)
        out["zero_pixel_exact"] = bool(torch.equal(y[1].cpu(), want))
    acc = mode == "acc"
    rg = bf.pitched(t["rg"], lo=4, hi=4) if acc else None
    nbytes = L.lgm_rmsnorm_bwd_workspace(npix, C)
    runs = []
    for _ in range(2):
        gx = bf.pitched(t["gx0"] if acc else None, shape=(npix, C))
        gg = bf.flat(t["gg0"] if acc else None, n=C)
        ws = bf.flat(n=nbytes // 4 + 4)
        args = (x.data_ptr(), _pitch(x), gy.data_ptr(), _pitch(gy), g.data_ptr(), gx.data_ptr(), _pitch(gx), int(acc), _ptr(rg), _pitch(rg),
                gg.data_ptr(), 1.0 if acc else 0.0, npix, C, ws.data_ptr())
        if mode == "deferred":
            desc = (ctypes.c_int64 * 8)()
            L.lgm_rmsnorm_bwd_deferred(*args, ctypes.addressof(desc), st)
            out["names"].append(_last())
            ops.wgrad_reduce_batch([tuple(desc)], dev)
        else:
            L.lgm_rmsnorm_bwd(*args, st)
            out["names"].append(_last())
        torch.cuda.synchronize()
        runs.append({"gx": gx, "gg": gg})
    _check(out, "backward", runs[0], pr.ref_b, pr.S_b)
    out["names"] = out["names"][:2] + ([] if out["names"][2] == out["names"][1] else [out["names"][2]])
    out["deterministic"] = all(bool(torch.equal(runs[0][k], runs[1][k])) for k in runs[0])
    out["guards"] = bf.intact()


def run_row(row, dev):
    out = {"names": [], "checks": [], "guards": None, "deterministic": None}
    (_run_rms if row["kind"] == "rms" else _run_gn)(row, problem(row), dev, out)
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("row", LEDGER, ids=row_id)
def test_norm_ledger_row(dev, parity, row):
    if row["plan"] is not None:
        B, C, H, W, G = row["geom"]
        assert gn_plan(B, H * W, C, G, 0) == gn_plan(B, H * W, C, G, 1) == row["plan"], row["why"]
    out = run_row(row, dev)
    assert tuple(out["names"]) == row["names"], f"{row_id(row)}: lgm_last_kernel reported {out['names']} ({row['why']})"
    assert out["checks"]
    for c in out["checks"]:
        parity(f"{' / '.join(row['names'])} {row_id(row).split('|', 2)[2]} {c['what']} [units of 2^-24 S]", c["score"], N.tolerance())
        assert c["score"] < N.tolerance_blocked(), (row_id(row), c, "over 4 x the float32 reference in torch's (blocked) order")
        assert c["rel"] < RTOL, (row_id(row), c)
    assert out["guards"] is True, f"{row_id(row)}: a NaN guard lane around an operand or an output was written"
    assert out["deterministic"] in (None, True), f"{row_id(row)}: two runs of the backward pass differ"
    assert out.get("zero_pixel_exact", True), f"{row_id(row)}: the all-zero pixel's output is not exactly the residual"
