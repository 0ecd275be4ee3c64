"""The workspace pool on the device: a buffer stays where it is while it is large enough (captured graphs hold raw pointers
into it), streams and tags have buffers of their own, the owners of a separator never share one, and a captured forward
still replays the same values after every workspace has grown and been replaced in its owner."""
import pytest
import torch

from xumx_slicq_amd import _lib
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu

MODELS = {"wiener1": dict(realtime=False, niter=1), "mixphase": dict(realtime=True)}


@pytest.fixture(scope="module")
def seps():
    from xumx_slicq_amd.separator import seeded_separator
    return {k: seeded_separator(**kw) for k, kw in MODELS.items()}


@pytest.fixture(scope="module")
def short():
    return synth_audio(9031, seed=7).cuda()


@pytest.fixture(scope="module")
def longer():
    return synth_audio(70000, seed=8).cuda()


def test_a_buffer_keeps_its_place_per_stream_and_tag():
    dev = torch.device("cuda")
    pool = _lib.Scratch()
    a = pool.get(dev, 4096)
    assert a.dtype == torch.uint8 and a.numel() == 4096 and a.device.type == "cuda"
    b = pool.get(dev, 1024)
    assert (b.data_ptr(), b.numel()) == (a.data_ptr(), 4096) and b is a
    c = pool.get(dev, 8192)
    assert c.numel() == 8192 and len(pool) == 1 and pool.tensors() == [c]
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, None)
    assert list(pool) == [key]
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        d = pool.get(dev, 8192)
    assert d.data_ptr() != c.data_ptr() and pool[key] is c and len(pool) == 2
    assert pool.get(dev, 8192, stream=other.cuda_stream) is d                        # the stream by pointer: the same entry
    e = pool.get(dev, 8192, tag="tail")
    assert e.data_ptr() not in (c.data_ptr(), d.data_ptr()) and pool[key] is c and len(pool) == 3
    assert pool.get(torch.device("cuda", torch.cuda.current_device()), 100) is c    # an explicit index is the same device
    assert pool.get(dev, 0, tag="nothing").numel() == _lib.Scratch.FLOOR == 256
    assert len(pool.tensors()) == 4


def _python_loop(sep, x):
    """``forward`` through the module API (the A/B arm of the native call): the arm that uses the engine's, the model's and the
    post-filter's workspaces."""
    sep.native = False
    try:
        return sep(x)
    finally:
        sep.__dict__.pop("native", None)


def test_the_owners_of_a_separator_do_not_alias(seps, short):
    from xumx_slicq_amd import phase
    sep = seps["wiener1"]
    want = sep(short)
    assert torch.equal(_python_loop(sep, short), want)
    torch.cuda.synchronize()
    held = sep._scratch_tensors()
    ids = {id(t) for t in held}
    assert len(ids) == len(held)
    eng = sep.nsgt.nsgt.nsgt
    for owner in (eng.scratch, sep.insgt.nsgt.nsgt.scratch, sep.xumx_model.scratch, phase.SCRATCH, sep._nws):
        assert owner.tensors() and all(id(t) in ids for t in owner.tensors())
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel()) for t in held)
    assert all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:])), spans


@pytest.mark.parametrize("model,arm", [("wiener1", "native"), ("mixphase", "native"), ("wiener1", "python")])
def test_a_captured_forward_survives_the_growth_of_every_workspace(seps, short, longer, model, arm):
    sep = seps[model]
    sep.drop_graphs()
    if arm == "python":
        sep.native = False
    try:
        first = sep.forward_graphed(short).clone()
        assert torch.equal(first, sep(short))
        before = {t.data_ptr(): t.numel() for t in sep._scratch_tensors()}
        want = sep(longer).clone()                  # replaces the buffers of the caller's stream ...
        assert torch.equal(sep.forward_graphed(longer), want)           # ... and a larger capture those of the capture stream
        after = {t.data_ptr(): t.numel() for t in sep._scratch_tensors()}
        assert set(before) - set(after), "no workspace was replaced: the longer calls did not grow any"
        assert sum(after.values()) > sum(before.values())
        again = sep.forward_graphed(short)
        assert len(sep._graphs) == 2
        torch.cuda.synchronize()
        assert torch.equal(again, first)
    finally:
        sep.__dict__.pop("native", None)
        sep.drop_graphs()
