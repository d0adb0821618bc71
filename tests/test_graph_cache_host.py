"""CPU: the cache of captured inference steps behind ``sampler._graph_chain`` and ``likelihood._graph_vlb`` - lookup, the drop of
an entry captured against storage the network no longer owns, the countdown after a failed capture, keys side by side, the
disabled and the device-less call, and the weak hold on the network.  No library, no device: the diffusion claims a device of
type "cuda", ``prepare_hip`` does nothing and both step classes are a fake that counts its constructions."""
import gc
import types
import weakref

import pytest

SHAPE = (2, 3, 16, 16)
FAILED = "[lgm_hip] {} graph capture unavailable (RuntimeError: no capture); eager launches\n"


class _Entry:
    """one entry point: ``call(gd, flag)`` with the two keys ``key(gd, False)`` / ``key(gd, True)``, and its word on stderr"""

    def __init__(self, word):
        from lgm_hip import likelihood as LK, sampler
        self.word = word
        if word == "sampler":
            self.call = lambda gd, flag=False: sampler._graph_chain(gd, SHAPE, flag)
            self.key = lambda gd, flag=False: sampler._graph_key(gd, SHAPE, flag, False, False, False)
        else:
            self.call = lambda gd, flag=False: LK._graph_vlb(gd, SHAPE, flag)
            self.key = lambda gd, flag=False: LK._vlb_key(gd, SHAPE, flag)


@pytest.fixture(params=["sampler", "likelihood"])
def entry(request):
    return _Entry(request.param)


@pytest.fixture
def fake(monkeypatch):
    """the class both ``_GraphedChain`` and ``_GraphedVLB`` are for this test: ``calls`` constructions tried, ``fail`` makes the
    next ones raise, an instance's ``ok`` is what its ``matches`` answers"""
    from lgm_hip import likelihood as LK, sampler

    class Step:
        calls, fail = 0, False

        def __init__(self, *args, **kw):         # (it keeps none of its arguments: the network stays weakly held)
            Step.calls += 1
            if Step.fail:
                raise RuntimeError("no capture")
            self.ok = True

        def matches(self, net):
            return self.ok

    monkeypatch.setattr(sampler, "_GraphedChain", Step)
    monkeypatch.setattr(LK, "_GraphedVLB", Step)
    monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "0")
    return Step


def _diffusion(device_type="cuda"):
    from models.generative.diffusion.ddpm import GaussianDiffusion, Unet
    net = Unet(dim=16, channels=3)
    gd = GaussianDiffusion(net, img_size=16, timesteps=12)
    gd.__dict__["betas"] = types.SimpleNamespace(device=types.SimpleNamespace(type=device_type))   # in front of the buffer
    net.prepare_hip = lambda device: None
    return gd


def test_repeated_call_returns_the_cached_step(entry, fake):
    from lgm_hip import sampler
    gd = _diffusion()
    first = entry.call(gd)
    assert isinstance(first, fake) and fake.calls == 1
    assert entry.call(gd) is first and fake.calls == 1, "a second call with the same key constructs nothing"
    assert sampler._GRAPHS[gd.model] == {entry.key(gd): first}


def test_stale_entry_is_dropped_and_rebuilt_once(entry, fake):
    from lgm_hip import sampler
    gd = _diffusion()
    first = entry.call(gd)
    first.ok = False
    second = entry.call(gd)
    assert isinstance(second, fake) and second is not first and fake.calls == 2
    assert sampler._GRAPHS[gd.model] == {entry.key(gd): second}, "exactly one new step, under the same key"
    assert entry.call(gd) is second and fake.calls == 2


def test_failed_capture_is_retried_after_the_countdown(entry, fake, capsys):
    from lgm_hip import sampler
    gd = _diffusion()
    fake.fail = True
    assert entry.call(gd) is None and fake.calls == 1
    assert capsys.readouterr().err == FAILED.format(entry.word)
    fake.fail = False
    for _ in range(sampler._CAPTURE_RETRY_AFTER):
        assert entry.call(gd) is None
    assert fake.calls == 1, "the builder is not called during the countdown"
    assert capsys.readouterr().err == ""
    step = entry.call(gd)
    assert isinstance(step, fake) and fake.calls == 2
    assert sampler._GRAPHS[gd.model] == {entry.key(gd): step}
    assert entry.call(gd) is step and fake.calls == 2


def test_a_stale_entry_whose_recapture_fails_counts_down_too(entry, fake, capsys):
    from lgm_hip import sampler
    gd = _diffusion()
    first = entry.call(gd)
    first.ok, fake.fail = False, True
    assert entry.call(gd) is None and fake.calls == 2
    assert capsys.readouterr().err == FAILED.format(entry.word)
    assert sampler._GRAPHS[gd.model] == {entry.key(gd): sampler._CAPTURE_RETRY_AFTER}, "the stale step is gone"


def test_keys_fail_retry_and_invalidate_independently(entry, fake, capsys):
    from lgm_hip import sampler
    gd = _diffusion()
    ka, kb = entry.key(gd, False), entry.key(gd, True)
    assert ka != kb
    fake.fail = True
    assert entry.call(gd, False) is None                       # key a fails ...
    fake.fail = False
    b = entry.call(gd, True)                                   # ... key b is built beside it
    assert isinstance(b, fake) and fake.calls == 2
    per = sampler._GRAPHS[gd.model]
    assert per == {ka: sampler._CAPTURE_RETRY_AFTER, kb: b}
    for _ in range(sampler._CAPTURE_RETRY_AFTER):
        assert entry.call(gd, False) is None and entry.call(gd, True) is b
    assert fake.calls == 2
    a = entry.call(gd, False)
    assert isinstance(a, fake) and fake.calls == 3 and per == {ka: a, kb: b}
    b.ok = False                                               # invalidating b leaves a alone
    b2 = entry.call(gd, True)
    assert b2 is not b and entry.call(gd, False) is a and fake.calls == 4 and per == {ka: a, kb: b2}
    assert capsys.readouterr().err == FAILED.format(entry.word), "one failure, one line"


def test_a_sampler_key_and_a_likelihood_key_share_the_network_entry(fake):
    from lgm_hip import likelihood as LK, sampler
    gd = _diffusion()
    chain, vlb = sampler._graph_chain(gd, SHAPE, True), LK._graph_vlb(gd, SHAPE, True)
    assert chain is not vlb and fake.calls == 2
    ks, kv = sampler._graph_key(gd, SHAPE, True, False, False, False), LK._vlb_key(gd, SHAPE, True)
    assert sampler._GRAPHS[gd.model] == {ks: chain, kv: vlb}
    vlb.ok = False
    assert sampler._graph_chain(gd, SHAPE, True) is chain and LK._graph_vlb(gd, SHAPE, True) is not vlb
    assert fake.calls == 3 and set(sampler._GRAPHS[gd.model]) == {ks, kv}


@pytest.mark.parametrize("how", ["disabled", "cpu"])
def test_disabled_or_device_less_call_touches_nothing(entry, fake, monkeypatch, how):
    from lgm_hip import sampler
    gd = _diffusion("cpu" if how == "cpu" else "cuda")
    if how == "disabled":
        monkeypatch.setenv("LGM_NO_SAMPLER_GRAPH", "1")
    assert entry.call(gd) is None and fake.calls == 0
    assert gd.model not in sampler._GRAPHS


def test_network_that_goes_away_takes_its_entry_along(entry, fake):
    from lgm_hip import sampler
    gc.collect()
    before = len(sampler._GRAPHS)
    gd = _diffusion()
    assert entry.call(gd) is not None
    net = weakref.ref(gd.model)
    assert net() in sampler._GRAPHS and len(sampler._GRAPHS) == before + 1
    del gd
    gc.collect()
    assert net() is None and len(sampler._GRAPHS) == before
