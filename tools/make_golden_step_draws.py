"""Record tests/golden/step_draws_host.json: what a training step of every diffusion variant draws, in which order, and what
it launches, as a checkout of the commit BEFORE the draws were folded into one routine per diffusion does it
(tests/step_draws.py holds the run; tests/test_step_draws_host.py compares the tree at hand with this record).  Runs on the CPU:
the library is a recorder.

Usage:  python tools/make_golden_step_draws.py --tree DIR [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="the checkout whose package is measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "step_draws_host.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for p in (tree, os.path.join(tree, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import lgm_hip
    import step_draws
    assert os.path.abspath(lgm_hip.__file__).startswith(tree), f"package {lgm_hip.__file__} is not the one of {tree}"
    out = step_draws.measure()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(a.out, {k: v["step0"]["launches"] for k, v in out.items()})


if __name__ == "__main__":
    main()
