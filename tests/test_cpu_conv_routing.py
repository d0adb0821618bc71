"""CPU: the host routing of the convolution family (lgm_hip/ops.py) with the library replaced by a recorder.  Every route
a layer can take through conv_xy / conv_yx, the statistics, weight-gradient and pair launchers: which entry points launch,
in which order, and what the KernelTimer records (family, FLOPs, bytes).  Queries (``*_supported``, ``*_workspace`` ...)
are answered but not asserted: their order is not part of the contract."""
import ctypes
import types

import pytest
import torch

from lgm_hip import ops

QUERIES = ("_supported", "_preferred", "_fits", "_workspace", "_floats")


class FakeLib:
    """Records every entry-point call.  Queries answer 1 (``*_supported``, ``*_preferred``, ``*_fits``) or 0 (sizes),
    launches 0; ``answers[name]`` overrides either (a value, or a callable of the arguments)."""

    def __init__(self):
        self.calls = []
        self.answers = {}

    def __getattr__(self, name):
        if not name.startswith("lgm_"):
            raise AttributeError(name)

        def call(*args):
            query = any(q in name for q in QUERIES)
            if not query:
                self.calls.append(f"{name}({args[0]})" if name == "lgm_wgrad_queue_enable" else name)
            a = self.answers.get(name)
            if callable(a):
                return a(*args)
            if a is not None:
                return a
            return 1 if query and not name.endswith(("_workspace", "_workspaces", "_floats", "_partial")) else 0
        return call


class FakeTimer:
    def __init__(self, calls):
        self.calls = calls

    def begin(self, name, flops, nbytes=0.0):
        self.calls.append(("begin", name, flops, nbytes))

    def end(self):
        self.calls.append(("end",))


class FakeFlat:
    """A registered flat buffer: the F(2x2) / F(4x4) operands of a slot at distinct fake addresses."""

    def __init__(self, total=4096):
        self.data = torch.zeros(total)
        self.total = total

    def wino_u(self, off, backward):
        return 0x100000 + 4 * off + (0x10000 if backward else 0)

    def wino4_u(self, off, backward):
        return 0x200000 + 4 * off + (0x10000 if backward else 0)


class FakeB3Flat:
    """A flat buffer with split-precision planes for the 3x3 slot at offset 0 (both orientations)."""

    def __init__(self, total=4096):
        self.data, self.data_t = torch.zeros(total), torch.zeros(total)
        self.planes, self.planes_t = torch.zeros(3 * total), torch.zeros(3 * total)
        self.total, self.pstride = total, total
        self._b3_slots = ({0}, {0})


def _desc_writer(pos, **fields):
    """An answer that writes ``fields`` (index -> value) into the int64 array passed as argument ``pos``."""
    def answer(*args):
        arr = (ctypes.c_int64 * 8).from_address(args[pos])
        for k, v in fields.items():
            arr[int(k[1:])] = v
        return 0
    return answer


@pytest.fixture
def env(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(ops, "lib", lambda: fake)
    monkeypatch.setattr(ops, "stream", lambda: 0)
    monkeypatch.setattr(ops, "TIMER", FakeTimer(fake.calls))
    for flag, v in (("WINO", True), ("WINO4", True), ("B3", False), ("POSTOPS", True), ("PLANES", True), ("BN_EPI", True),
                    ("GEMM1X1", False), ("WENG", False), ("WGRAD_QUEUE", True), ("WGRAD2", True),
                    ("WGRAD1X1_GROUP", True)):
        monkeypatch.setattr(ops, flag, v)
    # the module's live buffers and registrations: private to the test (a later GPU test must never see a CPU buffer)
    for name in ("_WS", "_PAIR_SLABS", "_GN_WS", "_WGRAD_WS", "_WGRAD_TABLES", "_WENG_U"):
        monkeypatch.setattr(ops, name, {})
    for name in ("_WS_RETIRED", "_WINO_FLATS", "_B3_FLATS"):
        monkeypatch.setattr(ops, name, [])
    ops.clear_plan_caches()
    fp = FakeFlat()
    ops.register_wino_flat(fp)
    fake.flat = fp
    yield fake
    ops.clear_plan_caches()


def _launches(fake):
    out, fake.calls[:] = list(fake.calls), []
    return out


def _work(g, k=1.0):
    return (k * ops._conv_flops(g), k * ops._conv_bytes(g))


def _nhwc(B, H, W, C):
    return torch.zeros(B, H, W, C)


G3 = (2, 8, 8, 16, 16, 3, 3, 1, 1)


def _g3():
    return ops.make_geom(*G3)


def _timed(fam, g, calls, k=1.0):
    return [("begin", fam) + _work(g, k)] + calls + [("end",)]


XY, YX = ("lgm_conv_xy", "igemm_xy"), ("lgm_conv_yx", "igemm_yx")


def _run(fake, yx, g, **kw):
    a = _nhwc(g.B, g.Ho, g.Wo, g.Nw) if yx else _nhwc(g.B, g.H, g.W, g.Cw)
    out = _nhwc(g.B, g.H, g.W, g.Cw) if yx else _nhwc(g.B, g.Ho, g.Wo, g.Nw)
    w = kw.pop("w", fake.flat.data.data_ptr())
    if yx:
        return ops.conv_yx(g, a, w, None, None, out, kw.pop("wt", None), **kw)
    return ops.conv_xy(g, a, w, None, None, out, **kw)


@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_winograd_and_direct_routes(env, monkeypatch, yx):
    g = _g3()
    fam = YX[1] if yx else XY[1]
    assert _run(env, yx, g) is None
    assert _launches(env) == _timed(fam, g, ["lgm_conv3x3_wino4"])
    monkeypatch.setattr(ops, "WINO4", False)
    ops.clear_plan_caches()
    _run(env, yx, g)
    assert _launches(env) == _timed(fam, g, ["lgm_conv3x3_wino"])
    monkeypatch.setattr(ops, "WINO", False)
    _run(env, yx, g)
    assert _launches(env) == _timed(fam, g, [YX[0] if yx else XY[0]])


@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_winograd_needs_an_operand_and_aligned_tensors(env, yx):
    g = _g3()
    fam = YX[1] if yx else XY[1]
    _run(env, yx, g, w=env.flat.data.data_ptr() + 2)           # not a slot address: no operand
    assert _launches(env) == _timed(fam, g, [YX[0] if yx else XY[0]])
    env.answers["lgm_conv3x3_wino_fits"] = 0                     # 32-bit offsets do not fit
    _run(env, yx, g)
    assert _launches(env) == _timed(fam, g, [YX[0] if yx else XY[0]])


@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_bf16x3_route(env, monkeypatch, yx):
    g = _g3()
    b3 = FakeB3Flat()
    ops.register_b3_flat(b3)
    monkeypatch.setattr(ops, "B3", True)
    w, wt = b3.data.data_ptr(), b3.data_t.data_ptr()
    _run(env, yx, g, w=w, wt=wt) if yx else _run(env, yx, g, w=w)
    assert _launches(env) == _timed(YX[1] if yx else XY[1], g, ["lgm_conv3x3_bf16x3"])
    if yx:      # the input gradient takes its planes from the transposed copy: none given, the direct kernel
        _run(env, yx, g, w=w)
        assert _launches(env) == _timed(YX[1], g, [YX[0]])


@pytest.mark.parametrize("postops", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_post_op_routes(env, monkeypatch, yx, postops):
    g = _g3()
    monkeypatch.setattr(ops, "POSTOPS", postops)
    mask = _nhwc(g.B, g.H, g.W, g.Cw) if yx else _nhwc(g.B, g.Ho, g.Wo, g.Nw)
    post = ops.make_post(ops.ACT_RELU, 0.0, mask, 0.2)
    _run(env, yx, g, post=post, post_mask=mask)
    d = YX[0] if yx else XY[0]
    want = [d + "_post"] if postops else [d, "lgm_act_fwd", "lgm_act_bwd"]
    assert _launches(env) == _timed(YX[1] if yx else XY[1], g, want)


@pytest.mark.parametrize("planes", [True, False], ids=["planes", "no_planes"])
@pytest.mark.parametrize("f4", [True, False], ids=["f44", "f22"])
@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_partial_routes(env, monkeypatch, yx, f4, planes):
    g = _g3()
    monkeypatch.setattr(ops, "PLANES", planes)
    monkeypatch.setattr(ops, "WINO4", f4)
    k = "lgm_conv3x3_wino4" if f4 else "lgm_conv3x3_wino"
    env.answers[k + "_workspace"] = env.answers["lgm_conv3x3_wino_workspace_partial"] = 1 << 16
    env.answers[k + "_partial"] = _desc_writer(-2, i0=3, i1=4096)
    r = _run(env, yx, g, partial=True)
    fam = YX[1] if yx else XY[1]
    if planes:
        assert r == (ops._WS[0].data_ptr(), 4096, 3, None)
        assert _launches(env) == _timed(fam, g, [k + "_partial"])
    else:
        assert r is None
        assert _launches(env) == _timed(fam, g, [k])


@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_gemm1x1_route(env, monkeypatch, yx):
    g = ops.make_geom(1, 32, 32, 128, 128, 1, 1, 1, 0)
    w = torch.zeros(128 * 128)
    _run(env, yx, g, w=w.data_ptr())
    d, fam = (YX if yx else XY)
    assert _launches(env) == _timed(fam, g, [d])
    monkeypatch.setattr(ops, "GEMM1X1", True)
    _run(env, yx, g, w=w.data_ptr())
    assert _launches(env) == _timed(fam, g, [d if yx else "lgm_weng_gemm_epi"])


@pytest.mark.parametrize("yx", [0, 1], ids=["xy", "yx"])
def test_engine_route(env, monkeypatch, yx):
    g = ops.make_geom(1, 8, 8, 32, 32, 4, 4, 2, 1)
    w = torch.zeros(32 * 16 * 32)
    d, fam = (YX if yx else XY)
    _run(env, yx, g, w=w.data_ptr())
    assert _launches(env) == _timed(fam, g, [d])                   # not registered
    monkeypatch.setattr(ops, "WENG", True)
    monkeypatch.setattr(ops, "WENG_MIN_FLOP", 0.0)
    assert ops.weng_register(w.data_ptr(), 32, 32, "cpu")
    _run(env, yx, g, w=w.data_ptr())
    s = "yx" if yx else "xy"
    assert _launches(env) == _timed(fam, g, [f"lgm_weng_f42_in_{s}", "lgm_weng_gemm", f"lgm_weng_f42_out_{s}_post"])
    _run(env, yx, g, w=w.data_ptr(), partial=True)                 # split planes: never the engine
    assert _launches(env) == _timed(fam, g, [d])


def test_conv_stats(env, monkeypatch):
    g = ops.make_geom(2, 8, 8, 32, 32, 4, 4, 2, 1)
    w = torch.zeros(32 * 16 * 32)
    for yx in (0, 1):
        a = _nhwc(g.B, g.Ho, g.Wo, g.Nw) if yx else _nhwc(g.B, g.H, g.W, g.Cw)
        out = _nhwc(g.B, g.H, g.W, g.Cw) if yx else _nhwc(g.B, g.Ho, g.Wo, g.Nw)
        env.answers["lgm_conv_stats_floats"] = 64
        st, tiles = ops.conv_stats(yx, g, a, w.data_ptr(), out)
        assert st.numel() == 64 and tiles == 0
        assert _launches(env) == _timed(YX[1] if yx else XY[1], g, ["lgm_conv_yx_stats" if yx else "lgm_conv_xy_stats"])


def test_conv_xy_stats(env, monkeypatch):
    g = _g3()
    x, y = _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16)
    w = env.flat.data.data_ptr()
    env.answers["lgm_gn_fwd_fused_supported"] = 1               # the fused GroupNorm serves this shape: not taken
    assert ops.conv_xy_stats(g, x, w, None, y, 4) is None
    ops.clear_plan_caches()
    env.answers["lgm_gn_fwd_fused_supported"] = 0
    env.answers["lgm_conv3x3_wino4_stats_floats"] = 96
    r = ops.conv_xy_stats(g, x, w, None, y, 4)
    assert r[0] == "stats" and r[1].numel() == 96 and r[2:] == (0, None)
    assert _launches(env) == _timed(XY[1], g, ["lgm_conv3x3_wino4_stats"])
    env.answers["lgm_conv3x3_wino_fits"] = 0
    ops._WINO_FITS.clear()
    assert ops.conv_xy_stats(g, x, w, None, y, 4) is None
    monkeypatch.setattr(ops, "WINO4", False)
    ops.clear_plan_caches()
    assert ops.conv_xy_stats(g, x, w, None, y, 4) is None
    assert _launches(env) == []


def test_conv_wgrad_plain_deferred_queued(env):
    g = _g3()
    gy, x = _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16)
    gw = torch.zeros(16 * 9 * 16)
    env.answers["lgm_conv_wgrad_workspace"] = 1024
    ops.conv_wgrad(g, gy, x, gw.data_ptr(), 0.0)
    assert _launches(env) == _timed("wgrad", g, ["lgm_conv_wgrad"])
    env.answers["lgm_conv_wgrad_deferred"] = _desc_writer(-2, i6=2)
    defer = []
    ops.conv_wgrad(g, gy, x, gw.data_ptr(), 0.0, defer=defer)
    assert _launches(env) == _timed("wgrad", g, ["lgm_conv_wgrad_deferred"])
    assert len(defer) == 1 and defer[0][6] == 2
    slab = ops._WGRAD_WS[(gw.data_ptr(), 1024)]
    assert slab.numel() == 1024 // 4 + 4
    ops.conv_wgrad(g, gy, x, gw.data_ptr(), 1.0, defer=defer, queue=True)
    assert _launches(env) == _timed("wgrad", g, ["lgm_wgrad_queue_enable(1)", "lgm_conv_wgrad_deferred",
                                                  "lgm_wgrad_queue_enable(0)"])
    assert ops._WGRAD_WS[(gw.data_ptr(), 1024)] is slab and len(defer) == 2
    ops.conv_wgrad(g, gy, x, gw.data_ptr(), 1.0, queue=True)      # queueing needs a deferred pass
    assert _launches(env) == _timed("wgrad", g, ["lgm_conv_wgrad"])
    ops.wgrad_queue_flush()
    assert _launches(env) == [("begin", "wgrad", 0.0, 0.0), "lgm_wgrad_queue_flush", ("end",)]


@pytest.mark.parametrize("kind", ["3x3", "1x1"])
def test_grouped_weight_gradients(env, kind):
    k = 3 if kind == "3x3" else 1
    geoms = [ops.make_geom(2, 8, 8, 16, 16, k, k, 1, k // 2), ops.make_geom(2, 8, 8, 32, 16, k, k, 1, k // 2)]
    launch = "lgm_conv3x3_wino_wgradn" if k == 3 else "lgm_wgrad1x1_group"
    supported = ops.wgrad_group_supported if k == 3 else ops.wgrad1x1_group_supported
    group = ops.conv_wgrad_group if k == 3 else ops.conv_wgrad1x1_group
    assert supported(geoms)
    env.answers[launch + "_supported"] = 0
    assert supported(geoms)                                      # cached answer
    ops.clear_plan_caches()
    assert not supported(geoms)
    env.answers["lgm_conv_wgrad_workspace"] = 512

    def sizes(n, arr, out):
        o = (ctypes.c_int64 * n).from_address(out)
        o[0], o[1] = 2048, 256                                   # the second is below the single-layer plan's 512
        return 0
    env.answers[launch + "_workspaces"] = sizes

    def launched(n, items, st):
        it = (ops.WgradItem * n).from_address(items)
        for i in range(n):
            (ctypes.c_int64 * 8).from_address(it[i].desc)[6] = 2 if i == 0 else 1
        return 0
    env.answers[launch] = launched
    gws = [torch.zeros(16 * k * k * 16), torch.zeros(16 * k * k * 32)]
    entries = [(g, _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, g.Cw), gw.data_ptr(), 0.0, None) for g, gw in zip(geoms, gws)]
    defer = []
    group(entries, defer)
    flops = sum(ops._conv_flops(g) for g in geoms)
    nbytes = sum(ops._conv_bytes(g) for g in geoms)
    assert _launches(env) == [("begin", "wgrad", flops, nbytes), launch, ("end",)]
    assert len(defer) == 1                                       # only the layer that split joins the reduction
    assert (gws[0].data_ptr(), 2048) in ops._WGRAD_WS and (gws[1].data_ptr(), 512) in ops._WGRAD_WS
    if k == 3:
        ops.conv_wgrad2(entries[0], entries[1], defer)
        assert _launches(env) == [("begin", "wgrad", flops, nbytes), launch, ("end",)]


def test_wgrad_queueable(env, monkeypatch):
    g3, g1 = _g3(), ops.make_geom(2, 8, 8, 16, 16, 1, 1, 1, 0)
    gy, x = _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16)
    assert ops.wgrad_queueable(g3, gy, x) and ops.wgrad1x1_queueable(g1, gy, x)
    assert not ops.wgrad1x1_queueable(g3, gy, x)
    assert not ops.wgrad_queueable(g3, gy[..., 1:], x) and not ops.wgrad1x1_queueable(g1, gy, x[..., 1:])
    monkeypatch.setattr(ops, "WGRAD2", False)
    monkeypatch.setattr(ops, "WGRAD1X1_GROUP", False)
    assert not ops.wgrad_queueable(g3, gy, x) and not ops.wgrad1x1_queueable(g1, gy, x)


@pytest.mark.parametrize("deferred", [False, True], ids=["now", "deferred"])
def test_conv_bwd_pair(env, deferred):
    g = _g3()
    gy, x, gx = _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16)
    gw = torch.zeros(16 * 9 * 16)
    w = env.flat.data.data_ptr()
    assert ops.conv_bwd_pair(g, gy, x, w, gw.data_ptr(), 0.0, None, None, None, gx) is False   # F(4x4) input gradient
    assert _launches(env) == []
    env.answers["lgm_conv3x3_wino4_preferred"] = 0
    ops.clear_plan_caches()

    def sizes(gp, partial, out):
        o = (ctypes.c_int64 * 2).from_address(out)
        o[0], o[1] = 1 << 16, 640
        return 0
    env.answers["lgm_conv3x3_wino_bwd_workspaces"] = sizes
    env.answers["lgm_conv3x3_wino_bwd"] = lambda *a: (_desc_writer(-2, i6=2)(*a) if a[-2] else 0) + \
        (_desc_writer(12, i0=2, i1=128)(*a) if a[12] else 0)
    defer = [] if deferred else None
    assert ops.conv_bwd_pair(g, gy, x, w, gw.data_ptr(), 0.0, None, defer, None, gx) is None
    assert _launches(env) == _timed("bwd_pair", g, ["lgm_conv3x3_wino_bwd"], 2.0)
    if deferred:
        assert len(defer) == 1 and ops._WGRAD_WS[(gw.data_ptr(), 640)].numel() == 640 // 4 + 4
    else:
        assert ops._PAIR_SLABS[0].numel() == 640 // 4 + 64 and not ops._WGRAD_WS
    r = ops.conv_bwd_pair(g, gy, x, w, gw.data_ptr(), 0.0, None, defer, None, gx, partial=True)
    assert r == (ops._WS[0].data_ptr(), 128, 2, None)
    _launches(env)
    env.answers["lgm_conv3x3_wino_bwd_supported"] = 0
    ops.clear_plan_caches()
    assert ops.conv_bwd_pair(g, gy, x, w, gw.data_ptr(), 0.0, None, defer, None, gx) is False
    assert _launches(env) == []


@pytest.mark.parametrize("postops", [True, False], ids=["fused", "separate"])
def test_conv_bwd_generic(env, monkeypatch, postops):
    monkeypatch.setattr(ops, "POSTOPS", postops)
    g = ops.make_geom(2, 8, 8, 16, 32, 1, 1, 1, 0)
    gy, x, gx = _nhwc(2, 8, 8, 32), _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16)
    gw = torch.zeros(32 * 16)
    w = torch.zeros(32 * 16)
    env.answers["lgm_conv_wgrad_workspace"] = 320
    env.answers["lgm_conv_bwd_pair"] = lambda *a: _desc_writer(-2, i6=2)(*a) if a[-2] else 0
    env.answers["lgm_conv_bwd_pair_post"] = lambda *a: _desc_writer(-3, i6=2)(*a) if a[-3] else 0
    ops.conv_bwd_generic(g, gy, x, w.data_ptr(), None, gw.data_ptr(), 0.0, None, None, None, gx)
    assert _launches(env) == _timed("bwd_pair", g, ["lgm_conv_bwd_pair"], 2.0)
    assert ops._PAIR_SLABS[0].numel() == 320 // 4 + 64
    defer = []
    ops.conv_bwd_generic(g, gy, x, w.data_ptr(), None, gw.data_ptr(), 0.0, None, defer, None, gx, queue=True)
    assert _launches(env) == _timed("bwd_pair", g, ["lgm_wgrad_queue_enable(1)", "lgm_conv_bwd_pair",
                                                     "lgm_wgrad_queue_enable(0)"], 2.0)
    assert len(defer) == 1 and (gw.data_ptr(), 320) in ops._WGRAD_WS
    post = ops.make_post(0, 0.0, gx, 0.0)
    ops.conv_bwd_generic(g, gy, x, w.data_ptr(), None, gw.data_ptr(), 0.0, None, defer, None, gx, post=post, post_mask=gx)
    want = ["lgm_conv_bwd_pair_post"] if postops else ["lgm_conv_bwd_pair", "lgm_act_bwd"]
    assert _launches(env) == _timed("bwd_pair", g, want, 2.0)
    assert len(defer) == 2


def test_batched_reduction_and_reducer(env):
    rows = [(1, 2, 3, 300, 0, 20, 2, 0), (4, 5, 6, 10, 0, 0, 3, 0)]
    ops.wgrad_reduce_batch(list(rows), "cpu")
    assert _launches(env) == [("begin", "wgrad", 0.0, 0.0), "lgm_wgrad_reduce_batch", ("end",)]
    ent = ops._WGRAD_TABLES[tuple(rows)]
    assert ent[0].tolist() == [list(rows[0]) + [0], list(rows[1]) + [2]]
    red = ops.make_reducer(rows, "cpu")
    assert red[0].tolist() == ent[0].tolist() and red[1:] == (2, 3)
    ops.launch_reducer(red)
    assert _launches(env) == ["lgm_wgrad_reduce_batch"]
    assert ops.make_reducer([], "cpu") is None and ops.wgrad_reduce_batch([], "cpu") is None


def test_clear_plan_caches_forgets_every_planner_answer(env, monkeypatch):
    """lgm_set_cu_margin / lgm_wino4_set_light change what the planners answer: clear_plan_caches() (run after either)
    must forget every cached answer - the shape-only ones too - and keep the live buffers."""
    monkeypatch.setattr(ops, "TIME_MLP", True)
    g, g1 = _g3(), ops.make_geom(2, 8, 8, 16, 16, 1, 1, 1, 0)
    gy, x = _nhwc(2, 8, 8, 16), _nhwc(2, 8, 8, 16)
    env.answers["lgm_conv3x3_wino4_stats_floats"] = 96
    env.answers["lgm_gn_fwd_fused_supported"] = 0
    ops.conv_xy_stats(g, x, env.flat.data.data_ptr(), None, gy, 4)
    monkeypatch.setattr(ops, "WINO4", False)            # F(2x2): the pair launch and its plans
    ops.conv_bwd_pair(g, gy, x, env.flat.data.data_ptr(), torch.zeros(4).data_ptr(), 0.0, None, [], None, x)
    for yx in (0, 1):
        _run(env, yx, g)
        _run(env, yx, g1, w=torch.zeros(256).data_ptr())
    ops._b3_supported(g, 0, 16)
    ops.wgrad_group_supported([g, g])
    ops.wgrad1x1_group_supported([g1, g1])
    gws = [torch.zeros(16 * 9 * 16) for _ in range(2)]
    ops.conv_wgrad_group([(g, gy, x, p.data_ptr(), 0.0, None) for p in gws], [])
    ops.conv_wgrad1x1_group([(g1, gy, x, p.data_ptr(), 0.0, None) for p in gws], [])
    ops.gn_planes_ok(2, 64, 16, 4)
    lin = types.SimpleNamespace(bias=object())
    assert ops.time_mlp_ok(16, 64, lin, lin)
    caches = ("_CONV_WS_BYTES", "_WINO_OK", "_WINO_WS", "_WINO4_OK", "_EPI_STATS", "_WINO_FITS", "_PAIR_OK", "_WG2_OK",
              "_WG2_WS", "_W1G_OK", "_W1G_WS", "_GN_PLANES_OK", "_B3_OK", "_TIME_MLP_OK")
    assert all(getattr(ops, n) for n in caches), [n for n in caches if not getattr(ops, n)]
    live = dict(ops._WGRAD_WS)
    assert live
    ops.clear_plan_caches()
    assert [n for n in caches if getattr(ops, n)] == []
    assert ops._WGRAD_WS.keys() == live.keys() and all(ops._WGRAD_WS[k] is v for k, v in live.items())

