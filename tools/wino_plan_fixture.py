#!/usr/bin/env python3
"""Host-side plan answers of the Winograd family, as a fixture: tests/golden/wino_plans.json.

Every value is an integer the library computes on the CPU (no GPU is opened): which geometries the F(4x4) / F(2x2) kernels
take, their split-K workspaces (hence the split counts), the F(4x4)-over-F(2x2) preference, the GroupNorm-statistics rows
and the weight-gradient workspaces - each under lgm_set_cu_margin 0 / 16 crossed with lgm_wino4_set_light -1 / 0 / 1.
tests/test_cpu_wino_plans.py compares the library it runs against with the committed file, value for value.

    python tools/wino_plan_fixture.py --write      regenerate tests/golden/wino_plans.json (sweep + environment slices)
    python tools/wino_plan_fixture.py --slice      print the slice of the sweep as JSON (the test runs this in a child
                                                   process per environment knob: the knobs are read once per process)

The fixture records what the planners answered when it was written; regenerate it only with a change that means to move a
plan, and say so.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightning-generative-models_amd"))
from lgm_hip import _lib  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "wino_plans.json")

BATCHES = (4, 8, 16, 32, 64, 128)
MAPS = ((4, 4), (8, 8), (16, 16), (8, 32), (16, 32), (32, 32), (64, 64), (24, 24))           # 24 x 24: refused
CHANNELS = ((32, 64), (64, 64), (64, 128), (128, 128), (256, 256), (256, 384), (512, 512), (768, 512), (48, 64))   # 48: refused
CONTEXTS = tuple((m, l) for m in (0, 16) for l in (-1, 0, 1))                                 # (CU margin, light mode)
SLICE_BATCHES = (16, 64)
# knobs the library reads once per process: each gets a child process that repeats the slice
ENV_CASES = ({"LGM_WINO4_LIGHT": "1"}, {"LGM_WINO4_SPLITS": "2"}, {"LGM_WINO4_LIGHT_BELOW": "64,32,16"},
             {"LGM_WINO4_TN_SLOWEST": "1"})

# (entry point, takes the direction yx)
_BY_DIRECTION = ("lgm_conv3x3_wino4_supported", "lgm_conv3x3_wino4_workspace", "lgm_conv3x3_wino4_preferred",
                 "lgm_conv3x3_wino4l_supported", "lgm_conv3x3_wino4l_workspace",
                 "lgm_conv3x3_wino_supported", "lgm_conv3x3_wino_workspace", "lgm_conv3x3_wino_workspace_partial")
_BY_GEOMETRY = ("lgm_conv3x3_wino4_wgrad_supported", "lgm_conv3x3_wino4_wgrad_workspace", "lgm_conv_wgrad_workspace")
QUERIES = tuple(f"{n}[yx={yx}]" for n in _BY_DIRECTION for yx in (0, 1)) + \
    ("lgm_conv3x3_wino4_stats_floats", "lgm_conv3x3_wino4_stats_floats:parts_per_image") + _BY_GEOMETRY


def load():
    """The library through plain ctypes (signatures from include/lgm_hip.h): plan queries need no HIP runtime set-up."""
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib.parse_header().items():
        fn = getattr(dll, name)
        fn.restype, fn.argtypes = res, args
    return dll


def answers(dll, B, H, W, C, N):
    g = ctypes.byref(_lib.ConvGeom(B, H, W, C, H, W, N, 3, 3, 1, 1))
    out = [int(getattr(dll, n)(g, yx)) for n in _BY_DIRECTION for yx in (0, 1)]
    parts = ctypes.c_int(-1)
    out.append(int(dll.lgm_conv3x3_wino4_stats_floats(g, ctypes.addressof(parts))))
    out.append(parts.value)
    out += [int(getattr(dll, n)(g)) for n in _BY_GEOMETRY]
    return out


def sweep(dll, batches=BATCHES):
    """One row per geometry: {"g": [B, H, W, C, N], "v": the distinct answer vectors (in QUERIES order), "c": which of them
    each of CONTEXTS got}."""
    rows = []
    try:
        for B in batches:
            for H, W in MAPS:
                for C, N in CHANNELS:
                    vecs, idx = [], []
                    for margin, light in CONTEXTS:
                        assert dll.lgm_set_cu_margin(margin) == 0 and dll.lgm_wino4_set_light(light) == 0
                        v = answers(dll, B, H, W, C, N)
                        if v not in vecs:
                            vecs.append(v)
                        idx.append(vecs.index(v))
                    rows.append({"g": [B, H, W, C, N], "v": vecs, "c": idx})
    finally:
        dll.lgm_set_cu_margin(-1)
        dll.lgm_wino4_set_light(-1)
    return rows


def env_key(env):
    return ",".join(f"{k}={v}" for k, v in sorted(env.items()))


def slice_in_child(env):
    """The slice as a fresh process answers it with `env` added to this process's environment."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--slice"], env={**os.environ, **env}, check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out)


def main():
    if "--slice" in sys.argv:
        json.dump(sweep(load(), SLICE_BATCHES), sys.stdout, separators=(",", ":"))
        return
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    doc = {"queries": list(QUERIES), "contexts": [list(c) for c in CONTEXTS], "rows": sweep(load()),
           "slice_batches": list(SLICE_BATCHES), "env": {env_key(e): slice_in_child(e) for e in ENV_CASES}}
    with open(FIXTURE, "w") as fh:      # one geometry per line
        fh.write('{"queries":%s,\n"contexts":%s,\n"slice_batches":%s,\n"rows":[\n' % tuple(
            json.dumps(doc[k], separators=(",", ":")) for k in ("queries", "contexts", "slice_batches")))
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in doc["rows"]))
        fh.write('\n],\n"env":{\n')
        fh.write(",\n".join('%s:[\n%s\n]' % (json.dumps(k), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
                            for k, rows in doc["env"].items()))
        fh.write("\n}}\n")
    print(f"{FIXTURE}: {len(doc['rows'])} geometries, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
