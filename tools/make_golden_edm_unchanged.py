"""Record tests/golden/diffusion_edm_unchanged.json: the bits and the launch trace of the sinusoidal (discrete-time) paths - one
eager DDPM training step, two graph-replayed ones, a DDIM chain - as a checkout of the commit BEFORE the Fourier time embedding
and elucidated diffusion computes them (tests/edm_unchanged.py holds the run; tests/test_hip_edm.py compares the tree at hand
with this record).  Needs a GPU and that checkout with its library built.

Usage:  python tools/make_golden_edm_unchanged.py --tree DIR [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="the checkout whose package and library are measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "diffusion_edm_unchanged.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for p in (tree, os.path.join(tree, "lightning-generative-models_amd")):
        sys.path.insert(0, p)
    import torch
    from lgm_hip import _lib
    import edm_unchanged
    assert torch.cuda.is_available(), "needs a GPU"
    assert os.path.abspath(_lib.LIB_PATH).startswith(tree), f"library {_lib.LIB_PATH} is not the one of {tree}"
    out = edm_unchanged.measure(torch.device("cuda", 0))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(a.out, len(out["step"]["trace"]), "launches in the step,", len(out["ddim"]["trace"]), "in the chain")


if __name__ == "__main__":
    main()
