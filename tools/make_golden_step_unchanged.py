"""Record tests/golden/diffusion_step_unchanged.json: the bits, the draws and the launch trace of one eager and two
graph-replayed training steps of every diffusion variant, as a checkout of the commit BEFORE the draws were folded into one
routine per diffusion computes them (tests/step_unchanged.py holds the run; tests/test_hip_step_unchanged.py compares the tree
at hand with this record).  The run is made twice: a kind is recorded where both agree; one whose runs differ is listed under
"unstable" with the fields that differed, and the record keeps its other fields.  Needs a GPU and that checkout with its
library built.

Usage:  python tools/make_golden_step_unchanged.py --tree DIR [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="the checkout whose package and library are measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "diffusion_step_unchanged.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for p in (tree, os.path.join(tree, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import _lib
    import step_unchanged
    assert torch.cuda.is_available(), "needs a GPU"
    assert os.path.abspath(_lib.LIB_PATH).startswith(tree), f"library {_lib.LIB_PATH} is not the one of {tree}"
    dev = torch.device("cuda", 0)
    first, second = step_unchanged.measure(dev), step_unchanged.measure(dev)
    unstable = {}
    for kind in first:
        fa, fb = step_unchanged.flatten(first[kind]), step_unchanged.flatten(second[kind])
        differ = sorted(k for k in fa if fa[k] != fb.get(k))
        if differ:
            unstable[kind] = differ
    assert len(unstable) <= 1 and "plain" not in unstable, f"the parent does not reproduce itself: {unstable}"
    with open(a.out, "w") as fh:
        json.dump({"kinds": first, "unstable": unstable}, fh, indent=1)
        fh.write("\n")
    print(a.out, "unstable:", unstable, {k: v["eager"]["launches"] for k, v in first.items()})


if __name__ == "__main__":
    main()
