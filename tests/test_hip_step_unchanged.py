"""GPU: every diffusion variant's training step - one eager, two graph-replayed - gives the bits, the draws and the launch
trace it gave on the commit before the draws were folded into one routine per diffusion
(tests/golden/diffusion_step_unchanged.json, recorded by tools/make_golden_step_unchanged.py; tests/step_unchanged.py is the
run on both sides)."""
import json
import os

import pytest
import torch

import step_unchanged

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "diffusion_step_unchanged.json")) as fh:
        return json.load(fh)


def test_the_record_holds_every_kind_and_the_plain_one_is_stable(golden):
    assert set(golden["kinds"]) == set(step_unchanged.KINDS)
    assert len(golden["unstable"]) <= 1 and "plain" not in golden["unstable"]


@pytest.mark.parametrize("kind", list(step_unchanged.KINDS))
def test_step_gives_the_recorded_bits_draws_and_trace(golden, kind):
    """Loss bits, sha-256 of gradient, parameters and EMA shadow, of every operand the step object holds after each replay,
    ``fast.mode``, length and hash of the eager launch trace: all of them, but the fields the recording commit did not
    reproduce itself (``unstable``).  Within the tree the eager step and the first replayed one - same seed, same batch, same
    coin - give the same loss bits."""
    assert torch.cuda.is_available()
    got = step_unchanged.measure(torch.device("cuda", 0), [kind])[kind]
    want, skip = step_unchanged.flatten(golden["kinds"][kind]), set(golden["unstable"].get(kind, ()))
    flat = step_unchanged.flatten(got)
    print(json.dumps(got, indent=1))
    assert set(flat) == set(want)
    assert {k: v for k, v in flat.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}
    assert got["eager"]["loss"] == got["graph"]["steps"][0]["loss"]
