"""The ledger of the attention kernels (csrc/attention.hip, attention_tiled.hip, linattn_mfma.hip): every route of
lgm_linattn_fwd / lgm_linattn_bwd, of lgm_attn_fwd / lgm_attn_bwd and of the fused LinearAttention tails (linattn_fused.hip)
is RUN through lgm_hip.ops at the smallest shape that reaches its edge, `lgm_last_kernel()` is compared with the row, and every output - ctx / ksum, out, lse, the qkv gradient and the
memory columns' gradient - is compared with float64 ELEMENTWISE in units of 2^-24 * S (oracle/attention.py; the tolerance is
four times what tests/test_cpu_attention_bounds.py measures on the float32 CPU evaluations).  The ratio of norms the per-op
tests use is put on record only: where a family makes a whole gradient a cancellation residue ("memmax", "spike") it says
nothing.  kmax is a maximum and must equal the reference bit for bit.  Operands and outputs are pitched views of
NaN-filled buffers whose guard lanes must stay untouched; outputs start as NaN; two runs of the backward pass must give equal
bits.

The input families (oracle.attention.la_inputs / fa_inputs) make the running maximum of the online-softmax kernels MOVE: a
key ramp that rises tile after tile, a largest key that is the very last one, a memory column above every pixel, a spike.

Rows whose kernel is reachable only under an environment switch (the library reads each once per process) run in a fresh
child process per switch, one at a time; a child that ends by signal, abort or timeout fails the test and no further child
starts in the session.

On the CPU (tests/test_cpu_attention_bounds.py) the worst float32 evaluation of the LinearAttention rows is ksum of the
n = 128 "memmax" row (1.75 units, torch's order) and of the full-attention rows lse of the n + M = 192 "memmax" row (2.46 units,
every order); the fused tails stay under 1.  The measured GPU values are in profiles/attention_ledger_parity.json
(LGM_PARITY_LOG): the worst kernel scores are ksum of the n = 35 "spike" row and lse of the same "memmax" row.

The completeness tests need no GPU."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":          # child process of test_switch_rows: the package is not on the path yet
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "lightning-generative-models_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from oracle import attention as A

DH = 32
NAMES = ("attn_small_fwd_kernel", "attn_small_bwd_kernel", "attn_fwd_kernel", "attn_bwd_kernel", "attn_tiled_fwd_kernel",
         "attn_tiled_bwd_kernel", "linattn_out_kernel", "linattn_bwd_mfma", "linattn_ctx_mfma<0>", "linattn_ctx_mfma<1>")
LA_NAMES = ("linattn_out_kernel", "linattn_bwd_mfma")        # the last launch of lgm_linattn_fwd / lgm_linattn_bwd
SMALL = ("attn_small_fwd_kernel", "attn_small_bwd_kernel")
ROWWISE = ("attn_fwd_kernel", "attn_bwd_kernel")
TILED = ("attn_tiled_fwd_kernel", "attn_tiled_bwd_kernel")


def LA(geom, family, why, **opts):
    return {"kind": "linattn", "geom": tuple(geom), "family": family, "names": LA_NAMES, "why": why, "env": None, "opts": opts}


def FT(geom, family, why):
    return {"kind": "la_fwd_tail", "geom": tuple(geom), "family": family, "names": (f"linattn_out_fused_kernel<{geom[1] // 32}>",),
            "why": why, "env": None, "opts": {}}


def BT(geom, family, blocks, why):
    return {"kind": "la_bwd_tail", "geom": tuple(geom), "family": family, "names": ("linattn_bwd_fused_kernel",), "why": why,
            "env": None, "opts": {"beta": 1.0, "blocks": blocks}}


def FA(names, geom, family, why, env=None, **opts):
    return {"kind": "attn", "geom": tuple(geom), "family": family, "names": names, "why": why, "env": env, "opts": opts}


# geometry = (B, heads, H, W, M).  opts: beta = 1: the memory gradient is added onto existing content, and the deferred form
# (reduced by wgrad_reduce_batch) must give the direct form's bits; gmem_offset: the memory gradient's pointer is moved by
# that many floats (not 16-byte aligned); odd: a qkv pitch that is no multiple of 4 floats on an unaligned base.
LEDGER = [
    # ---- LinearAttention core: linattn_ctx_mfma<0> appends the M memory columns as rows n .. n + M - 1 of 128-row tiles
    LA((2, 3, 1, 1, 4), "plain", "n = 1: the softmax over n is carried by the memory columns; odd head count"),
    LA((2, 4, 9, 14, 4), "ascending", "n = 126: memory columns are rows 126..129, across the tile boundary"),
    LA((1, 2, 8, 16, 4), "memmax", "n = 128: the second tile holds only the four memory columns, and the maximum moves there"),
    LA((2, 1, 3, 43, 0), "late", "n = 129, M = 0: one live row in the last tile carries the maximum; heads = 1"),
    LA((1, 4, 16, 16, 16), "ascending", "n = 256: three tiles, M = 16, the maximum moves at each"),
    LA((2, 2, 5, 7, 4), "spike", "n = 35: half-empty single tile"),
    LA((2, 4, 9, 14, 4), "ascending", "mem_kv gradient not 16-byte aligned: the is_mem tile of linattn_bwd_mfma + lgm_colsum",
       gmem_offset=1),
    LA((2, 4, 9, 14, 4), "ascending", "gmem_beta = 1 on existing content; the deferred form gives the same bits", beta=1.0),
    # ---- full attention, attn_small_*: aligned operands, n <= 64
    FA(SMALL, (2, 3, 1, 1, 0), "plain", "one key: out = v, the q and k gradients are pure cancellation, and S > 0"),
    FA(SMALL, (2, 2, 3, 5, 4), "spike", "n = 15, four memory rows"),
    FA(SMALL, (1, 4, 8, 8, 16), "late", "n = 64, nk = 80: the upper limit of the route"),
    # ---- attn_fwd_kernel / attn_bwd_kernel: one thread per row
    FA(ROWWISE, (1, 3, 5, 13, 4), "ascending", "n = 65: the first n past the small route"),
    FA(ROWWISE, (2, 2, 8, 16, 16), "late", "n = 128, nk = 144: the upper limit of this route"),
    FA(ROWWISE, (2, 2, 3, 5, 4), "plain", "a qkv pitch that is no multiple of 4: the alignment gate of the small route sends it here",
       odd=True),
    # ---- attn_tiled_*: key tiles of 64, memory rows first
    FA(TILED, (1, 2, 3, 43, 0), "late", "n = 129: three query tiles, the last with one query"),
    FA(TILED, (1, 3, 4, 47, 4), "memmax", "n + M = 192: exactly three key tiles"),
    FA(TILED, (1, 2, 7, 27, 4), "late", "n + M = 193: the last key tile holds one key, and it is the maximum", beta=1.0),
    FA(TILED, (1, 1, 12, 16, 16), "peaked", "three whole query tiles, M = 16"),
    # ---- the fused tails of LinearAttention, (B, C, H, W) with heads = 4 and M = 4.  Forward: ao, o2 = to_out[0](ao) and
    # y = RMSNorm(o2) + x from one launch; the saved ctx / kmax / ksum must be those of the unfused forward
    FT((2, 64, 9, 14), "ascending", "C = 64: n = 126, the memory columns straddle the tile boundary; two images"),
    FT((1, 128, 8, 16), "memmax", "C = 128: n = 128, one full pixel tile"),
    FT((1, 256, 3, 43), "late", "C = 256: n = 129, the second item holds one pixel, and it carries the maximum"),
    # backward: gxn, to_qkv's weight gradient (beta = 1 on existing content) and the memory gradient, direct and deferred.
    # plan_blocks: items = B * cdiv(n, 128), at most 256 blocks, per = cdiv(items, blocks) items each
    BT((3, 64, 9, 14), "spike", 3, "small layout: 3 items, one per block"),
    BT((257, 64, 1, 2), "plain", 129, "257 items, 2 per block, 129 blocks, the last with one item"),
    BT((87, 64, 1, 257), "ascending", 131, "3 tiles per image, 261 items, 2 per block, 131 blocks: blocks cross image boundaries and the "
       "last has one item"),
    # ---- switch rows
    FA(ROWWISE, (2, 2, 3, 5, 4), "plain", "LGM_NO_SMALL_ATTN=1: the one-thread-per-row pair at a small-route shape",
       env="LGM_NO_SMALL_ATTN=1"),
    FA(TILED, (2, 3, 1, 1, 0), "plain", "LGM_TILED_ATTN=1: one query, one key", env="LGM_TILED_ATTN=1"),
    FA(TILED, (1, 2, 6, 10, 4), "plain", "LGM_TILED_ATTN=1: n + M = 64, one exact key tile", env="LGM_TILED_ATTN=1"),
]


def row_id(row):
    o = row["opts"]
    tag = "".join(f"-{k}" for k in ("beta", "gmem_offset", "odd") if o.get(k) and row["kind"] in ("linattn", "attn")) + (f"-{row['env']}" if row["env"] else "")
    return f"{row['names'][0]}|{'x'.join(map(str, row['geom']))}|{row['family']}{tag}"


_PROBLEMS = {}


def problem(row):
    """The row's operands, float64 results and scales, never changed by a test (one row at a time is kept)."""
    key = row_id(row)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()
        if row["kind"] in ("linattn", "attn"):
            _PROBLEMS[key] = A.Problem(row["kind"], row["geom"], row["family"], seed=LEDGER.index(row),
                                       beta=row["opts"].get("beta", 0.0))
        else:
            _PROBLEMS[key] = A.TailProblem(row["kind"], row["geom"], row["family"], seed=LEDGER.index(row))
    return _PROBLEMS[key]


def registry_names():
    import ctypes
    from lgm_hip import _lib
    D = _lib.lib()._dll
    D.lgm_kernel_name.restype = ctypes.c_char_p
    return sorted({D.lgm_kernel_name(i).decode() for i in range(D.lgm_kernel_name_count())})


# ---- completeness (no GPU) ------------------------------------------------------------------------------------------------
def test_every_attention_kernel_name_has_a_ledger_row():
    reg = registry_names()
    names = [n for n in reg if n.startswith(("attn_", "linattn_ctx_mfma", "linattn_bwd_mfma", "linattn_out_kernel"))]
    assert sorted(names) == sorted(NAMES), "names the attention launchers can note"
    fused = {n for n in reg if n.startswith(("linattn_out_fused_kernel", "linattn_bwd_fused_kernel"))}
    assert len(fused) == 4
    keys = {n for r in LEDGER for n in r["names"]}
    assert fused <= keys, "every fused tail the library can note has a row"
    keys -= fused
    # linattn_ctx_mfma<0> / <1> are the FIRST launch of every LinearAttention entry point: lgm_last_kernel() reports the
    # launch that follows them, and the same rows' ctx / ksum / kmax and gradients check them
    assert keys | {"linattn_ctx_mfma<0>", "linattn_ctx_mfma<1>"} == set(NAMES)
    assert len({row_id(r) for r in LEDGER}) == len(LEDGER)
    assert all(r["why"] for r in LEDGER)


def test_every_row_sits_on_the_route_it_is_written_for():
    """the host-side route of lgm_attn_fwd / attn_bwd_impl restated: tiled above 128 queries, small up to 64 with aligned
    operands, else one thread per row; switch rows only differ by their switch"""
    for r in LEDGER:
        if r["kind"] != "attn":
            continue
        n = r["geom"][2] * r["geom"][3]
        want = TILED if n > 128 else SMALL if n <= 64 and not r["opts"].get("odd") else ROWWISE
        if r["env"]:
            assert want == SMALL and r["names"] == (TILED if "TILED" in r["env"] else ROWWISE)
        else:
            assert r["names"] == want, row_id(r)


# ---- running one row ---------------------------------------------------------------------------------------------------------
NAN = float("nan")


class Buffers:
    """Device buffers of one row, every one between NaN guards: pitched NHWC views [B, H, W, C] (pitch C + lo + hi) and flat
    vectors (32 guard floats in front, ``shift`` more to move the base off 16 bytes).  Outputs start as NaN."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def nhwc(self, src=None, shape=None, lo=4, hi=4):
        B, H, W, C = shape if src is None else src.shape
        buf = torch.full((B, H, W, C + lo + hi), NAN, device=self.dev)
        view = buf[..., lo:lo + C]
        if src is not None:
            view.copy_(src)
        self.all.append((buf, lo, C))
        return view

    def flat(self, src=None, n=None, shift=0):
        n = n if src is None else src.numel()
        buf = torch.full((max(n, 4) + 64 + shift,), NAN, device=self.dev)
        view = buf[32 + shift:32 + shift + n]
        if src is not None:
            view.copy_(src.reshape(-1))
        self.all.append((buf, 32 + shift, n))
        return view

    def intact(self):
        return all(bool(torch.isnan(b[..., :lo]).all()) and bool(torch.isnan(b[..., lo + n:]).all()) for b, lo, n in self.all)


def _last():
    from lgm_hip import ops
    k = ops.lib()._dll.lgm_last_kernel()
    return k.decode() if k else ""


def _check(out, fam, stage, got, ref, S):
    for k in S:
        if k not in got:
            continue
        g = got[k].detach().cpu().reshape(ref[k].shape)
        out["checks"].append({"what": f"{stage} {k}", "score": A.forward_error_units(g, ref[k], S[k]), "rel": A.rel(g, ref[k]),
                              "tol": A.tolerance(fam)})


def _pack(t, la, keys):
    """[B, 3 | 1, heads, ...] operands -> NHWC [B, n, len(keys) * hidden] with channel = which * hidden + head * 32 + d"""
    x = torch.stack([t[k] for k in keys], 1)                         # [B, w, heads, 32, n] | [B, w, heads, n, 32]
    x = x.permute(0, 4, 1, 2, 3) if la else x.permute(0, 3, 1, 2, 4)
    return x.reshape(x.shape[0], x.shape[1], -1)


def _unpack(x, la, w, heads):
    """NHWC [B, H, W, w * hidden] -> [B, w, heads, 32, n] | [B, w, heads, n, 32]"""
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    x = x.detach().cpu().reshape(B, n, w, heads, DH)
    return x.permute(0, 2, 3, 4, 1) if la else x.permute(0, 2, 3, 1, 4)


def _rows(x):
    """a pitched NHWC view -> [B * n, C] on the CPU"""
    return x.detach().cpu().reshape(-1, x.shape[-1])


def _run_fwd_tail(row, dev, out):
    from lgm_hip import ops
    pr, t = problem(row), problem(row).t
    B, C, H, W = row["geom"]
    heads, M, hidden = 4, 4, 4 * DH
    bf = Buffers(dev)
    qkv = bf.nhwc(_pack(t, True, ("q", "k", "v")).reshape(B, H, W, 3 * hidden), lo=4, hi=8)
    x = bf.nhwc(t["x"].reshape(B, H, W, C), lo=4, hi=4)
    mem, wout, bout, g = (bf.flat(t[k]) for k in ("mem", "wout", "bout", "g"))
    ao, o2, y = bf.nhwc(shape=(B, H, W, hidden)), bf.nhwc(shape=(B, H, W, C), lo=8, hi=4), bf.nhwc(shape=(B, H, W, C), lo=4, hi=8)
    assert ops.linattn_fwd_fused_ok(heads, DH, C, qkv, x, wout.data_ptr(), bout.data_ptr(), g.data_ptr(), any_size=True)
    ctx, kstat = ops.linattn_fwd_fused(qkv, mem.data_ptr(), heads, DH, M, wout.data_ptr(), bout.data_ptr(), g.data_ptr(), x,
                                       ao, o2, y)
    out["names"].append(_last())
    torch.cuda.synchronize()
    _check(out, row["kind"], "forward", {"ao": _rows(ao), "o2": _rows(o2), "y": _rows(y)}, pr.ref, pr.S)
    out["kmax_exact"] = bool(torch.equal(kstat[0].cpu(), pr.ref["kmax"].float()))
    od = bf.nhwc(shape=(B, H, W, hidden))
    ctx2, kstat2 = ops.linattn_fwd(qkv, mem.data_ptr(), heads, DH, M, od)
    torch.cuda.synchronize()
    out["saved_equal"] = bool(torch.equal(ctx, ctx2)) and bool(torch.equal(kstat, kstat2))
    out["guards"] = bf.intact()


def _run_bwd_tail(row, dev, out):
    from lgm_hip import ops
    pr, t = problem(row), problem(row).t
    B, C, H, W = row["geom"]
    heads, M, hidden = 4, 4, 4 * DH
    bf = Buffers(dev)
    qkv = bf.nhwc(_pack(t, True, ("q", "k", "v")).reshape(B, H, W, 3 * hidden), lo=4, hi=8)
    gout = bf.nhwc(_pack(t, True, ("gout",)).reshape(B, H, W, hidden), lo=8, hi=4)
    xn = bf.nhwc(t["xn"].reshape(B, H, W, C), lo=4, hi=4)
    mem, wt = bf.flat(t["mem"]), bf.flat(t["wqkv"].t().contiguous())          # the weight's transposed copy [C][3 * hidden]
    od = bf.nhwc(shape=(B, H, W, hidden))
    ctx, kstat = ops.linattn_fwd(qkv, mem.data_ptr(), heads, DH, M, od)
    runs = []
    for deferred in (False, True, False):
        gxn, gw, gm = bf.nhwc(shape=(B, H, W, C)), bf.flat(t["gw0"]), bf.flat(t["gm0"])
        assert ops.linattn_bwd_fused_ok(heads, DH, C, qkv, gout, xn, wt.data_ptr(), gw.data_ptr(), gm.data_ptr())
        dw, dm = ([], []) if deferred else (None, None)
        ops.linattn_bwd_fused(qkv, mem.data_ptr(), gout, ctx, kstat, xn, wt.data_ptr(), heads, DH, M, gxn, gw.data_ptr(), 1.0, dw,
                              gm.data_ptr(), 1.0, dm)
        name = _last()
        if deferred:
            assert len(dw) == 1 and len(dm) == 1
            out["blocks"] = int(dw[0][6])
            ops.wgrad_reduce_batch(dw + dm, dev)
        torch.cuda.synchronize()
        runs.append((name, gxn, gw, gm))
    out["names"].append(runs[0][0])
    for stage, r in (("backward", runs[0]), ("backward deferred", runs[1])):
        _check(out, row["kind"], stage, {"gxn": _rows(r[1]), "gw": r[2], "gmem": r[3]}, pr.ref, pr.S)
    same = lambda a, b: a[0] == b[0] and all(bool(torch.equal(u, v)) for u, v in zip(a[1:], b[1:]))
    out["deterministic"], out["deferred_equal"] = same(runs[0], runs[2]), same(runs[0], runs[1])
    out["guards"] = bf.intact()


def run_row(row, dev):
    from lgm_hip import ops
    out = {"row": row_id(row), "names": [], "checks": [], "guards": None, "deterministic": None, "kmax_exact": None,
           "deferred_equal": None, "saved_equal": None, "blocks": None}
    if row["kind"] in ("la_fwd_tail", "la_bwd_tail"):
        (_run_fwd_tail if row["kind"] == "la_fwd_tail" else _run_bwd_tail)(row, dev, out)
        return out
    pr, o = problem(row), row["opts"]
    la, t, fam = row["kind"] == "linattn", pr.t, row["kind"]
    B, heads, H, W, M = row["geom"]
    hidden, beta = heads * DH, o.get("beta", 0.0)
    lo, hi = (1, 6) if o.get("odd") else (4, 8)
    bf = Buffers(dev)
    qkv = bf.nhwc(_pack(t, la, ("q", "k", "v")).reshape(B, H, W, 3 * hidden), lo=lo, hi=hi)
    gout = bf.nhwc(_pack(t, la, ("gout",)).reshape(B, H, W, hidden), lo=8, hi=4)
    mem = bf.flat(t["mem"]) if M else bf.flat(n=4)                 # (M = 0: never read, but a pointer is required)
    od = bf.nhwc(shape=(B, H, W, hidden), lo=4, hi=4)
    if la:
        ctx, kstat = ops.linattn_fwd(qkv, mem.data_ptr(), heads, DH, M, od)
        got = {"ctx": ctx, "ksum": kstat[1], "out": _unpack(od, la, 1, heads)[:, 0]}
    else:
        lse = ops.attn_fwd(qkv, mem.data_ptr(), heads, DH, M, od)
        got = {"out": _unpack(od, la, 1, heads)[:, 0], "lse": lse}
    out["names"].append(_last())
    torch.cuda.synchronize()
    _check(out, fam, "forward", got, pr.ref, {k: pr.S[k] for k in ("ctx", "ksum", "out", "lse") if k in pr.S})
    if la:
        out["kmax_exact"] = bool(torch.equal(kstat[0].cpu(), pr.ref["kmax"].float())) and \
            bool(torch.equal(pr.ref["kmax"].float().double(), pr.ref["kmax"]))

    def backward(defer=None):
        gq = bf.nhwc(shape=(B, H, W, 3 * hidden), lo=4, hi=4)
        gm = bf.flat(t["gm0"] if beta else None, n=max(t["mem"].numel(), 4), shift=o.get("gmem_offset", 0))
        if la:
            ops.linattn_bwd(qkv, mem.data_ptr(), gout, ctx, kstat, heads, DH, M, gq, gm.data_ptr(), beta, defer=defer)
        else:
            ops.attn_bwd(qkv, mem.data_ptr(), od, gout, lse, heads, DH, M, gq, gm.data_ptr(), beta, defer=defer)
        name = _last()
        if defer is not None:
            assert len(defer) == 1, "one reducer row for the memory gradient"
            ops.wgrad_reduce_batch(defer, dev)                          # (empties the list)
        torch.cuda.synchronize()
        return (name, gq, gm) if M else (name, gq)                      # (M = 0: no memory gradient is written)

    runs = [backward(), backward()]
    out["names"].append(runs[0][0])
    gotb = {"gqkv": _unpack(runs[0][1], la, 3, heads), "gmem": runs[0][-1]}
    _check(out, fam, "backward", gotb, pr.ref, {k: pr.S[k] for k in ("gqkv", "gmem") if k in pr.S})
    out["deterministic"] = runs[1][0] == runs[0][0] and all(bool(torch.equal(a, b)) for a, b in zip(runs[0][1:], runs[1][1:]))
    if beta:
        name, gq, gm = backward(defer=[])
        out["deferred_equal"] = name == runs[0][0] and bool(torch.equal(gq, runs[0][1])) and bool(torch.equal(gm, runs[0][2]))
    out["guards"] = bf.intact()
    return out


def judge(row, out, parity):
    """The assertions of one row, from the record its run left (in this process or in a child)."""
    assert tuple(out["names"]) == row["names"], f"{row_id(row)}: lgm_last_kernel reported {out['names']} ({row['why']})"
    kind = row["kind"]
    want = {"la_fwd_tail": {"forward ao", "forward o2", "forward y"},
            "la_bwd_tail": {f"{st} {k}" for st in ("backward", "backward deferred") for k in ("gxn", "gw", "gmem")},
            "linattn": {"forward ctx", "forward ksum", "forward out", "backward gqkv"},
            "attn": {"forward out", "forward lse", "backward gqkv"}}[kind]
    if kind in ("linattn", "attn") and row["geom"][4]:
        want = want | {"backward gmem"}
    assert {c["what"] for c in out["checks"]} == want
    for c in out["checks"]:
        assert c["tol"] == A.tolerance(kind)
        parity.record(f"{row_id(row)} {c['what']} [ratio of norms]", rel=c["rel"])
        parity(f"{row_id(row)} {c['what']} [units of 2^-24 S]", c["score"], c["tol"])
    assert out["guards"] is True, f"{row_id(row)}: a NaN guard lane around an operand or an output was written"
    assert out["deterministic"] is (None if kind == "la_fwd_tail" else True), f"{row_id(row)}: two runs of the backward pass differ"
    assert out["kmax_exact"] is (True if kind in ("linattn", "la_fwd_tail") else None), \
        f"{row_id(row)}: kmax is not the exact column maximum"
    assert out["deferred_equal"] is (True if row["opts"].get("beta") else None), \
        f"{row_id(row)}: the deferred reduction differs from the direct one"
    assert out["saved_equal"] is (True if kind == "la_fwd_tail" else None), \
        f"{row_id(row)}: the fused forward saves another ctx / kmax / ksum (or writes another out) than the unfused one"
    assert out["blocks"] == row["opts"].get("blocks"), f"{row_id(row)}: {out['blocks']} blocks ({row['why']})"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in LEDGER if r["env"] is None], ids=row_id)
def test_attention_ledger_row(dev, parity, monkeypatch, row):
    from lgm_hip import ops
    monkeypatch.setattr(ops, "LA_FUSED", True)
    monkeypatch.setattr(ops, "LA_FUSED_MIN_ITEMS", 0)   # the size gate of the fused backward is a performance choice, not a limit
    judge(row, run_row(row, dev), parity)


SWITCHES = sorted({r["env"] for r in LEDGER if r["env"]})
_CHILD_DIED = []


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
def test_switch_rows(parity, switch):
    """every row of one environment switch in a fresh child process (the library reads a switch once per process)"""
    assert not _CHILD_DIED, f"an earlier child died ({_CHILD_DIED[0]}): no further child is started in this session"
    rows = [r for r in LEDGER if r["env"] == switch]
    env = dict(os.environ)
    key, val = switch.split("=")
    env[key] = val
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", switch], env=env, capture_output=True,
                             text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(f"{switch}: timeout")
        raise
    if res.returncode != 0:
        _CHILD_DIED.append(f"{switch}: exit status {res.returncode}")
    assert res.returncode == 0, res.stderr[-2000:]
    outs = {o["row"]: o for o in json.loads(res.stdout.strip().splitlines()[-1])}
    assert sorted(outs) == sorted(row_id(r) for r in rows)
    for r in rows:
        judge(r, outs[row_id(r)], parity)


def _child(switch):
    key, val = switch.split("=")
    assert os.environ.get(key) == val
    dev = torch.device("cuda", 0)
    outs = [run_row(r, dev) for r in LEDGER if r["env"] == switch]
    for o in outs:
        for c in o["checks"]:
            if math.isinf(c["score"]):
                c["score"] = 1e300
    print(json.dumps(outs))


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
