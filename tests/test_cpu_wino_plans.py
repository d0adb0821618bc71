"""CPU: the host planners of the Winograd family answer what tests/golden/wino_plans.json recorded (tools/wino_plan_fixture.py
wrote it and names the sweep).  Which geometries the F(4x4) forms and the F(2x2) kernels take, the split-K workspaces (hence
the split counts), the F(4x4) preference, the GroupNorm-statistics rows and the weight-gradient workspaces, under
lgm_set_cu_margin 0 / 16 x lgm_wino4_set_light -1 / 0 / 1 - integers, compared for equality."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wino_plan_fixture", os.path.join(ROOT, "tools", "wino_plan_fixture.py"))
fx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fx)


@pytest.fixture(scope="module")
def golden():
    with open(fx.FIXTURE) as fh:
        doc = json.load(fh)
    # the fixture was written for the sweep the tool still describes
    assert doc["queries"] == list(fx.QUERIES) and doc["contexts"] == [list(c) for c in fx.CONTEXTS]
    assert doc["slice_batches"] == list(fx.SLICE_BATCHES)
    return doc


def _expand(row):
    return [row["v"][i] for i in row["c"]]


def _compare(got, want, what):
    assert [r["g"] for r in got] == [r["g"] for r in want], f"{what}: another sweep than the fixture's"
    for g, w in zip(got, want):
        for (margin, light), gv, wv in zip(fx.CONTEXTS, _expand(g), _expand(w)):
            diff = {q: (a, b) for q, a, b in zip(fx.QUERIES, gv, wv) if a != b}
            assert not diff, f"{what}: B, H, W, C, N = {g['g']}, cu_margin {margin}, light {light}: (got, recorded) {diff}"


def test_the_sweep_covers_every_class_and_the_refused_cases(golden):
    rows = golden["rows"]
    assert len(rows) == len(fx.BATCHES) * len(fx.MAPS) * len(fx.CHANNELS)
    q = {name: i for i, name in enumerate(fx.QUERIES)}
    took = {(r["g"][1], r["g"][2]) for r in rows if any(v[q["lgm_conv3x3_wino4_supported[yx=0]"]] for v in r["v"])}
    assert took == set(fx.MAPS) - {(24, 24)}                      # 32-tile classes 3, 2, 1, 0 and the light-only 8 x 32
    f44 = [i for name, i in q.items() if "_wino4" in name and "wgrad" not in name]     # (F(2x2) has its own, wider rules)
    for r in rows:
        if (r["g"][1], r["g"][2]) == (24, 24) or r["g"][3] == 48:
            assert not any(v[i] for v in r["v"] for i in f44), r["g"]


def test_plans_match_the_recorded_ones(golden):
    _compare(fx.sweep(fx.load()), golden["rows"], "in process")


@pytest.mark.parametrize("env", fx.ENV_CASES, ids=fx.env_key)
def test_plans_under_an_environment_knob_match_the_recorded_ones(golden, env):
    """The knobs are read once per process: a child process repeats a slice of the sweep with the knob set."""
    _compare(fx.slice_in_child(env), golden["env"][fx.env_key(env)], fx.env_key(env))


def test_the_environment_knobs_move_plans(golden):
    """...so that the slices above do exercise them.  (LGM_WINO4_TN_SLOWEST only reorders the units of a launch: no query
    shows it, its slice equals the plain one.)"""
    plain = [r for r in golden["rows"] if r["g"][0] in fx.SLICE_BATCHES]
    for key, rows in golden["env"].items():
        same = [_expand(a) for a in rows] == [_expand(b) for b in plain]
        assert same == (key == "LGM_WINO4_TN_SLOWEST=1"), key
