"""CPU: what the fold of the training step's host side named - the graph layout ``GraphedDDPMStep`` chooses per
configuration, and ``Unet.bucket_ranges()`` as the one source of the exchange ranges, on the eager and on the graphed path.
The recorder and the fakes are those of tests/test_step_trace_host.py."""
import pytest
import torch

from test_step_trace_host import BUCKETS, HALVES, LAYOUTS, WHOLE, _names, session  # noqa: F401  (session: the fixture)


def _ready(calls):
    return [args for name, args in calls if name == "ready"]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layout_per_configuration(session, layout):
    graph = session.graph
    assert (graph.LAYOUT_ONE, graph.LAYOUT_TWO, graph.LAYOUT_BUCKETS) == (WHOLE, HALVES, BUCKETS)
    one_graph, pipeline, with_sync, groups = LAYOUTS[layout]
    session.mp.setattr(graph, "_ONE_GRAPH", one_graph)
    session.mp.setattr(graph, "_STEP_PIPELINE", pipeline)
    fast, batch = session.fast("plain", True, with_sync)
    session.run(fast, batch, 0)
    gs = fast.graphed
    assert gs.layout == groups and gs.pipeline == pipeline and len(gs.graphs) == len(groups)
    buckets = fast.net.bucket_ranges()
    assert gs.ranges == [[r for k in group for r in buckets[k]] for group in groups]


def test_the_phases_are_one_ordered_tuple():
    from models.generative.diffusion.ddpm import Unet
    assert [p.__name__ for p in Unet.BACKWARD_PHASES] == ["_backward_up", "_backward_mid", "_backward_down", "_backward_time"]
    net = Unet(dim=16, channels=3)
    net.prepare_hip("cpu")
    assert len(net.bucket_ranges()) == len(Unet.BACKWARD_PHASES)


@pytest.mark.parametrize("pipeline", [False, True], ids=["graphs", "pipeline"])
def test_bucket_ranges_is_the_only_source_of_the_exchange_ranges(session, pipeline):
    """another cut of the same buffer, returned by a patched ``bucket_ranges()``: the eager backward, the graphed step and
    the pipelined step's Adam slices all follow it"""
    session.mp.setattr(session.graph, "_STEP_PIPELINE", pipeline)

    def recut(fast):
        net = fast.net
        (a, b), (c, t) = net.bucket_ranges()[0]
        (h, _), = net.bucket_ranges()[2]
        cut = [[(c, t), (a, a + 8), (a + 8, b)], [(b, c)], [(h + 4, a), (h, h + 4)], [(4, h), (0, 4)]]
        net.bucket_ranges = lambda: cut
        return cut
    eager, batch = session.fast("plain", False, True)
    cut = recut(eager)
    flat = [r for b in cut for r in b]
    assert _ready(session.run(eager, batch, 0)) == flat
    fast, batch = session.fast("plain", True, True)
    assert recut(fast) == cut
    session.run(fast, batch, 0)
    assert fast.graphed.ranges == cut
    step = session.run(fast, batch, 1)
    assert _ready(step) == flat
    if pipeline:
        assert [args[4] for name, args in step if name == "lgm_adam_step"] == [hi - lo for lo, hi in flat]
    else:
        assert _names(step).count("lgm_adam_step") == 1
    assert torch.equal(fast.graphed.x, batch[0])
