"""The equalities between the forward Wiener-EM entry points, at arena level on a two-block table small enough to run in a
blink: the masked form is bitwise the two-step form, and one iteration through the iteration entry points (either method) is
bitwise the plain call.  Every kernel behind them takes its arithmetic from csrc/wiener_math.h.

Blocks (F = 3, T = 4) and (F = 5, T = 10) at S = 6 are rows of 24 and 60 frames: with ``win_len`` = 16 that is 2 and 4 windows
with tails of 8 and 12 frames.  Batch item 3 is forty times louder, so the window maxima (hence ``ma`` > 1) differ between the
batch groups when ``batch_group`` = 2 and are shared over the batch when it is 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES, B, S, WIN = [(3, 4), (5, 10)], 4, 6, 16


@pytest.fixture(scope="module")
def arenas():
    from xumx_slicq_amd.arena import BlockTable
    table = BlockTable(SHAPES)
    g = torch.Generator().manual_seed(20261018)
    X = torch.randn(table.numel(2 * B, S), generator=g)
    for Xb in table.views(X, (B, 2), S):
        Xb[3] *= 40.0
    masks = torch.rand(table.numel(8 * B, S, complex_=False), generator=g).clamp_(1e-3, 1 - 1e-3)
    Y0 = torch.empty(table.numel(8 * B, S))
    for Yb, mb, Xb in zip(table.views(Y0, (4, B, 2), S), table.views(masks, (4, B, 2), S, complex_=False), table.views(X, (B, 2), S)):
        Yb.copy_(mb[..., None] * Xb[None])                  # single fp32 products: what the EM passes form on the way in
    assert float(X.abs().max()) > 100.0                     # ma = max(1, 0.1 max|x|) > 1 in the loud windows
    return table, X.cuda(), masks.cuda(), Y0.cuda()


def _iter_entry(table, X, masks, Y, batch_group, niter, method):
    """xsq_wiener_em_iter / xsq_wiener_em_masked_iter called directly (``wiener_em_arena`` routes niter = 1 to the plain call)."""
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.phase import METHODS, _tables, _workspace
    F, T = _tables(table)
    geometry = (len(table), F.ctypes.data, T.ctypes.data)
    nbytes = _lib.lib.xsq_wiener_iter_workspace(*geometry, B, S, WIN, niter, METHODS[method])
    assert nbytes > 0
    ws = _workspace(X.device, nbytes)
    tail = (B, S, WIN, batch_group)
    if masks is None:
        rc = _lib.lib.xsq_wiener_em_iter(*geometry, X.data_ptr(), Y.data_ptr(), *tail, niter, METHODS[method], ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr())
    else:
        rc = _lib.lib.xsq_wiener_em_masked_iter(*geometry, X.data_ptr(), masks.data_ptr(), Y.data_ptr(), *tail, None, niter,
                                                METHODS[method], ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "iteration entry point")


@pytest.mark.parametrize("batch_group", [0, 2])
def test_forward_entry_points_agree_bitwise_at_one_iteration(arenas, batch_group):
    from xumx_slicq_amd.phase import wiener_em_arena, wiener_em_masked_arena
    table, X, masks, Y0 = arenas
    two_step = Y0.clone()
    wiener_em_arena(table, X, two_step, B, S, WIN, batch_group, niter=1)
    assert torch.isfinite(two_step).all() and not torch.equal(two_step, Y0)
    from_masks = torch.full_like(Y0, float("nan"))           # only written
    wiener_em_masked_arena(table, X, masks, from_masks, B, S, WIN, batch_group, niter=1)
    assert torch.equal(from_masks, two_step)
    for method in ("looped", "resident"):
        y = Y0.clone()
        _iter_entry(table, X, None, y, batch_group, 1, method)
        assert torch.equal(y, two_step), method
        y = torch.full_like(Y0, float("nan"))
        _iter_entry(table, X, masks, y, batch_group, 1, method)
        assert torch.equal(y, two_step), method
    if batch_group == 2:                                     # the quiet group has its own window maxima
        shared = Y0.clone()
        wiener_em_arena(table, X, shared, B, S, WIN, 0, niter=1)
        assert not torch.equal(shared, two_step)
