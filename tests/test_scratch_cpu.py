"""The Python host side's three helpers, without a device: the workspace pool (``_lib.Scratch``), the checked native call
(``_lib.call``) and the checked size query (``_lib.workspace_bytes``)."""
import copy
import pickle

import pytest
import torch

from xumx_slicq_amd import _lib

DEV = torch.device("cuda", 3)          # an index only: nothing below touches a device


class HostScratch(_lib.Scratch):
    """The pool with its allocator replaced: host memory, and a record of every allocation."""
    allocated = []

    @staticmethod
    def _allocate(nbytes, device):
        HostScratch.allocated.append((nbytes, device))
        return torch.empty(nbytes, dtype=torch.uint8)


@pytest.fixture
def pool():
    HostScratch.allocated = []
    return HostScratch()


def test_the_key_is_device_index_stream_and_tag(pool):
    a = pool.get(DEV, 4096, stream=11)
    assert list(pool) == [(3, 11, None)] and a.numel() == 4096 and a.dtype == torch.uint8
    b = pool.get(DEV, 4096, stream=11, tag="tail")
    c = pool.get(DEV, 4096, stream=12)
    d = pool.get(torch.device("cuda", 1), 4096, stream=11)
    assert set(pool) == {(3, 11, None), (3, 11, "tail"), (3, 12, None), (1, 11, None)}
    assert len({t.data_ptr() for t in (a, b, c, d)}) == 4
    assert pool.get(DEV, 4096, stream=11) is a and pool.get(DEV, 4096, stream=11, tag="tail") is b
    assert {t.data_ptr() for t in pool.tensors()} == {t.data_ptr() for t in (a, b, c, d)} and len(pool.tensors()) == 4


def test_a_buffer_grows_and_never_shrinks(pool):
    a = pool.get(DEV, 4096, stream=0)
    assert pool.get(DEV, 1024, stream=0) is a and pool.get(DEV, 4096, stream=0) is a
    b = pool.get(DEV, 8192, stream=0)
    assert b.numel() == 8192 and pool.tensors() == [b] and len(pool) == 1          # exactly what was asked for, one entry
    assert pool.get(DEV, 100, stream=0) is b
    assert [n for n, _ in HostScratch.allocated] == [4096, 8192]
    # one floor for a request of no bytes, and a later real request replaces it
    z = pool.get(DEV, 0, stream=5)
    assert z.numel() == _lib.Scratch.FLOOR == 256
    assert pool.get(DEV, 0, stream=5) is z and pool.get(DEV, 256, stream=5) is z and pool.get(DEV, 257, stream=5).numel() == 257


def test_the_old_buffer_is_released_before_the_new_one_is_allocated(pool):
    seen = []

    class Watching(HostScratch):
        @staticmethod
        def _allocate(nbytes, device):
            seen.append(list(w.values()))
            return torch.empty(nbytes, dtype=torch.uint8)
    w = Watching()
    w.get(DEV, 64, stream=0)
    w.get(DEV, 128, stream=0)
    assert seen == [[None], [None]]


def test_a_copy_or_pickle_of_a_pool_is_an_empty_pool(pool):
    pool.get(DEV, 64, stream=0)
    pool[(7, 0)] = "stand-in"
    for c in (copy.deepcopy(pool), pickle.loads(pickle.dumps(pool)), copy.deepcopy({"owner": pool})["owner"]):
        assert type(c) is HostScratch and c == {} and c.tensors() == [] and c is not pool
    plain = pickle.loads(pickle.dumps(_lib.Scratch({(0, 0, None): None})))
    assert type(plain) is _lib.Scratch and plain == {}
    assert len(pool) == 2


@pytest.fixture(scope="module")
def unmix():
    from xumx_slicq_amd.separator import build_models
    return build_models(device="cpu")[0]


def test_a_copy_of_an_owner_gets_an_empty_pool_of_its_own(unmix):
    from xumx_slicq_amd.transforms import NSGTBase
    eng = NSGTBase("bark", 262, 32.9, device="cpu").nsgt
    blk = unmix.sliced_umx[0]
    for owner, name in ((unmix, "_ws"), (eng, "_ws"), (blk, "_block_ws")):
        mine = getattr(owner, name)
        assert type(mine) is _lib.Scratch
        mine[(7, 0)] = "workspace"
        try:
            for c in (copy.deepcopy(owner), pickle.loads(pickle.dumps(owner))):
                theirs = getattr(c, name)
                assert theirs == {} and type(theirs) is type(mine) and theirs is not mine
        finally:
            mine.pop((7, 0))
    assert unmix.scratch is unmix._ws and eng.scratch is eng._ws


def test_the_delegating_names_reach_the_owners_pools(unmix, monkeypatch):
    from xumx_slicq_amd import phase
    from xumx_slicq_amd.transforms import NSGTBase
    monkeypatch.setattr(_lib.Scratch, "_allocate", staticmethod(lambda nbytes, device: torch.empty(nbytes, dtype=torch.uint8)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 77})())
    eng = NSGTBase("bark", 262, 32.9, device="cpu").nsgt
    held = dict(phase.SCRATCH)
    try:
        for get, pool in ((eng.workspace, eng._ws), (unmix._workspace, unmix._ws), (phase._workspace, phase.SCRATCH)):
            ws = get(DEV, 512)
            assert pool[(3, 77, None)] is ws and ws.numel() == 512 and get(DEV, 100) is ws
    finally:
        phase.SCRATCH.clear()
        phase.SCRATCH.update(held)
        unmix._ws.clear()
        eng._ws.clear()


def test_device_index():
    assert _lib.device_index(torch.device("cuda", 5)) == 5 and _lib.device_index(torch.device("cuda:0")) == 0


def test_call_raises_naming_the_entry_point():
    with pytest.raises(_lib.XsqError) as e:
        _lib.call("xsq_plan_num_blocks", None)
    assert str(e.value).startswith("xsq_plan_num_blocks")
    with pytest.raises(_lib.XsqError) as e:
        _lib.call("xsq_cdae_forward_xin", None, None, 1, 3, None, None, None, 0, None, 0)
    assert str(e.value).startswith("xsq_cdae_forward_xin failed")
    assert _lib.call("xsq_profile_reset") is None                                   # status 0: nothing raised, nothing returned
    with pytest.raises(AttributeError):
        _lib.call("xsq_no_such_entry_point")


def test_workspace_bytes_names_the_query_and_reports_no_stale_message():
    assert _lib.workspace_bytes("xsq_sdr_loss_workspace", 1, 100) == _lib.lib.xsq_sdr_loss_workspace(1, 100) > 0
    with pytest.raises(_lib.XsqError) as e:
        _lib.workspace_bytes("xsq_sdr_loss_workspace", 0, 100)
    assert str(e.value).startswith("xsq_sdr_loss_workspace: ")
    # this query sets no text of its own: the hint stands in, whatever an earlier call left in the library's buffer
    assert _lib.lib.xsq_plan_num_blocks(None) < 0 and _lib.last_error()
    with pytest.raises(_lib.XsqError) as e:
        _lib.workspace_bytes("xsq_sdr_loss_workspace", 0, 100, why="bad shape B=0 n=100")
    assert str(e.value) == "xsq_sdr_loss_workspace: bad shape B=0 n=100"
    # this one does: its own message is reported
    with pytest.raises(_lib.XsqError) as e:
        _lib.workspace_bytes("xsq_ideal_workspace", None, 1, 9031, 0, 5000)
    assert str(e.value).startswith("xsq_ideal_workspace: ") and "null" in str(e.value)


def test_plan_switches_are_one_table_all_set_at_construction(monkeypatch):
    from xumx_slicq_amd import transforms
    assert list(transforms._PLAN_SWITCHES) == ["fft_backend", "band_radix4", "short_inline", "packed_fft"]
    assert all(setter == f"xsq_plan_set_{name}" and setter in _lib.EXPORTED for name, (setter, _) in transforms._PLAN_SWITCHES.items())
    monkeypatch.delenv("XSQ_SHORT_INLINE", raising=False)
    eng = transforms.NSGTBase("bark", 262, 32.9, device="cpu").nsgt
    assert (eng._fft_backend, eng._band_radix4, eng._short_inline, eng._packed_fft) == (0, True, False, False)
    monkeypatch.setenv("XSQ_SHORT_INLINE", "1")
    assert transforms.NSGTBase("bark", 262, 32.9, device="cpu").nsgt._short_inline is True
    # without a handle a setter only records; the values reach a handle through _apply
    eng.set_fft_backend(1), eng.set_band_radix4(False), eng.set_short_inline(True), eng.set_packed_fft(True)
    assert (eng._fft_backend, eng._band_radix4, eng._short_inline, eng._packed_fft) == (1, False, True, True)
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    eng._apply("h")
    assert calls == [("xsq_plan_set_fft_backend", ("h", 1)), ("xsq_plan_set_band_radix4", ("h", 0)),
                     ("xsq_plan_set_short_inline", ("h", 1)), ("xsq_plan_set_packed_fft", ("h", 1))]
    # a live handle is told first, and a value it refuses is not kept
    eng._handles[0] = "h"
    try:
        def refuse(name, *args):
            raise _lib.XsqError(name)
        monkeypatch.setattr(_lib, "call", refuse)
        eng.set_packed_fft(True)                                                    # unchanged: no call
        with pytest.raises(_lib.XsqError):
            eng.set_packed_fft(False)
        assert eng._packed_fft is True
    finally:
        eng._handles.clear()
