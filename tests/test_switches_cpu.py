"""The A/B switches of the whole-call layer (xumx_slicq_amd/separator.py: SWITCHES, switch, Separator._graph_key): one table, one reader,
and a graph key that holds every switch of the table in exactly one of its two parts.  No device."""
import os

import pytest

from xumx_slicq_amd.separator import SWITCHES, switch


class Bare:
    pass


@pytest.fixture
def clean_env():
    names = [env for _, env, _, _ in SWITCHES.values() if env]
    saved = {n: os.environ.pop(n) for n in names if n in os.environ}
    yield
    for n in names:
        os.environ.pop(n, None)
    os.environ.update(saved)


def test_every_entry_is_classified():
    """An entry without a graph-drop classification (or with anything but a bool there) fails here, and in the reader."""
    assert len(SWITCHES) >= 13
    for name, entry in SWITCHES.items():
        assert len(entry) == 4, name
        owner, env, default, drops = entry
        assert owner in ("separator", "model"), name
        assert env is None or (isinstance(env, str) and env.startswith("XSQ_")), name
        assert type(default) in (bool, int, str), name
        assert env is None or type(default) is bool, name          # the "0" rule yields a bool
        assert type(drops) is bool, name


@pytest.mark.parametrize("name", list(SWITCHES))
def test_reader(name, clean_env):
    _, env, default, _ = SWITCHES[name]
    obj = Bare()
    assert switch(obj, name) == default and type(switch(obj, name)) is type(default)
    if env:
        for text, want in (("0", False), ("1", True), ("", True), ("00", True), ("no", True)):
            os.environ[env] = text
            assert switch(obj, name) is want, (text, want)
        os.environ[env] = "0" if default else "1"                   # the environment now says the opposite of the default
    other = {bool: lambda v: not v, int: lambda v: v + 3, str: lambda v: v + "-x"}[type(default)](default)
    for value in (other, default):                                   # the attribute wins, whatever the environment says
        setattr(obj, name, value)
        assert switch(obj, name) == value and type(switch(obj, name)) is type(default)
    delattr(obj, name)                                               # (del sep.packed_fft)
    assert switch(obj, name) == ((not default) if env else default)
    setattr(obj, name, other)
    obj.__dict__.pop(name, None)                                     # (sep.__dict__.pop("native", None))
    assert switch(obj, name) == ((not default) if env else default)
    if env:
        del os.environ[env]
        assert switch(obj, name) == default


def test_unknown_name_raises():
    obj = Bare()
    obj.nonesuch = 1
    with pytest.raises(KeyError):
        switch(obj, "nonesuch")
    with pytest.raises(KeyError):
        switch(obj, "XSQ_NATIVE_FORWARD")


def test_none_is_a_value_not_absence(clean_env):
    """An attribute set to None is read as a value of the switch's type, as the spelled-out reads did: off for a bool,
    a TypeError for an int; only a missing attribute falls through to the environment and the default."""
    obj = Bare()
    obj.native, obj.max_stack = None, None
    assert switch(obj, "native") is False
    with pytest.raises(TypeError):
        switch(obj, "max_stack")


class FakeModel(Bare):
    sliced_umx = ()

    def _version(self):
        return 3


class FakeSeparator(Bare):
    """What ``Separator._graph_key`` reads besides the switches."""
    chunk_size, niter, softmask, residual = 1000, 1, False, False

    def __init__(self):
        self.xumx_model = FakeModel()

    def _fused(self):
        return "fused"

    def _packed_fft(self):
        return "packed"


class FakeAudio:
    shape, device = (1, 2, 10), type("D", (), {"index": 0})()


# positions 8 onward of the tuple the key replaced: a change of one of these drops the captured forwards
INVALIDATING = {"fuse_phasemix", "fuse_whiten", "wiener_masked", "packed_fft", "native", "max_item_slices", "winograd", "niter_method"}
COEXIST = {"precision", "overlap_tail", "batch_chunks", "max_stack", "pass_streams"}


def test_every_switch_is_in_exactly_one_part_of_the_graph_key(clean_env):
    from xumx_slicq_amd.separator import Separator
    sep = FakeSeparator()
    key = Separator._graph_key(sep, FakeAudio())
    assert key.device == 0 and key.coexist[:2] == ((1, 2, 10), 1000)
    assert key.invalidating[:5] == (3, (), 1, False, False)
    coexist, invalidating = dict(key.coexist[2:]), dict(key.invalidating[5:])
    assert set(coexist) == COEXIST and set(invalidating) == INVALIDATING                 # (literal: independent of the table)
    assert COEXIST | INVALIDATING == set(SWITCHES) and not COEXIST & INVALIDATING
    assert len(key.coexist) == 2 + len(COEXIST) and len(key.invalidating) == 5 + len(INVALIDATING)
    assert {n for n, e in SWITCHES.items() if e[3]} == INVALIDATING
    # two switches enter as what the call makes of them, the others as read
    assert invalidating.pop("fuse_phasemix") == "fused" and invalidating.pop("packed_fft") == "packed"
    assert {**coexist, **invalidating} == {n: e[2] for n, e in SWITCHES.items() if n not in ("fuse_phasemix", "packed_fft")}
    # each owner's attribute moves its own entry, in its own part, and nothing else
    for name, (owner, _, default, drops) in SWITCHES.items():
        if name in ("fuse_phasemix", "packed_fft"):
            continue
        other = {bool: lambda v: not v, int: lambda v: v + 3, str: lambda v: v + "-x"}[type(default)](default)
        right, wrong = FakeSeparator(), FakeSeparator()
        setattr(right if owner == "separator" else right.xumx_model, name, other)
        setattr(wrong.xumx_model if owner == "separator" else wrong, name, other)
        k2 = Separator._graph_key(right, FakeAudio())
        assert (k2.coexist != key.coexist) == (not drops) and (k2.invalidating != key.invalidating) == drops, name
        assert dict((k2.invalidating if drops else k2.coexist)[5 if drops else 2:])[name] == other
        assert Separator._graph_key(wrong, FakeAudio()) == key, name
