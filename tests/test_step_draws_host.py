"""CPU: every diffusion variant's training step draws what it drew, in the order it drew it, and launches what it launched -
against tests/golden/step_draws_host.json, recorded by tools/make_golden_step_draws.py on a checkout of the commit before the
draws were folded into one routine per diffusion (tests/step_draws.py is the run on both sides)."""
import json
import os

import pytest

import step_draws


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "step_draws_host.json")) as fh:
        return json.load(fh)


def test_the_record_holds_every_kind(golden):
    assert set(golden) == set(step_draws.KINDS)


@pytest.mark.parametrize("kind", list(step_draws.KINDS))
def test_step_draws_and_launches_are_the_recorded_ones(golden, kind):
    """The eager ``forward`` + ``backward``, ``p_losses`` with every operand given (it draws nothing) and two steps of
    ``DDPMFastStep``: the sequence of random calls with the bits each returned, the operands the network and the step object
    hold, the number of launches and the hash over entry points and scalar arguments."""
    traces = {}
    want, got = golden[kind], step_draws.measure([kind], traces)[kind]
    if got != want:                              # what it drew and held, and the launches of every run that differs
        print(json.dumps(got, indent=1))
        for run, calls in traces.items():
            if (got[run]["launches"], got[run]["trace"]) != (want[run]["launches"], want[run]["trace"]):
                print(f"--- {kind} {run}: {len(calls)} launches")
                print("\n".join(f"{name}{args}" for name, args in calls))
    for run in ("forward", "p_losses", "step0", "step1"):
        for field in ("draws", "operands", "launches", "trace"):
            assert got[run][field] == want[run][field], (kind, run, field)
    assert got["p_losses"]["draws"] == [] and got["step1"]["draws"] == []
    assert got == want
