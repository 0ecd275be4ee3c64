"""The FFT band engine (csrc/band_fft.h) on the device at the edges of its FFT classes and lengths: the made plan of
tests/test_longband_edges_cpu.py -- every class filled (2 m = N, Lg 512 .. 16384, the engine's maximum) and entered (Lg = 2 N + 4), the
smallest band (324) as the DC band, the Nyquist band at full length, blocks of F = 2 and 3, windows of one weight at every entry --
through both transforms, the masked and the remix inverse and both adjoints.  That module owns the plan, the shapes (n = 2 h + 1:
S = 3, and n = 7 h + 123: S = 5 with a ragged tail) and the helpers, and holds on the CPU that this rule reports a band with one wrong
entry.

Rule, metric and helper are those of tests/test_logscale_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err`` / ``band_rel_err``, per band for
the analyses and per block or row for the syntheses; E the fp32 CPU oracle's error against float64 (oracle/ref64.py) on the same input;
M per stage the smallest power of two at least twice the worst ratio measured on MI355X (profiles/longband_edges_parity.json), at most
``M_CAP``.

Wall time of the module on MI355X: 5 s for its 10 tests in one process (the slowest, the forward with the device plan's creation and
the one-block inverse with its 16-row float64 references, 1.5 and 0.8 s; the forward adjoint with its table build 0.3 s; every other
test 0.1 s or less).  No stage needs an M above 4, and nothing failed at any edge: no change to the library came of it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref64
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables
from test_autograd_cpu import F32, F64, autograd_forward_adjoint, forward_adjoint_closed_form
from test_longband_edges_cpu import (BLOCKS, audio, band_labels, block_labels, edge_plan, flat, lengths, one_band_rows, one_block_rows,
                                     random_blocks)
from test_sdr_cpu import adjoint_closed_form, adjoint_window

pytestmark = pytest.mark.gpu

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/longband_edges_parity.json)
M = {
    "forward": 2,                  # 0.82  (both shapes: band 17, Lg 16372, which also has the largest E; the other engine bands 0.63 .. 0.77, the DC band 0.65)
    "inverse": 4,                  # 1.24  (one band of a block alone: band 9, f 2 of 3; one block alone 1.00, block 14, T 16372; all blocks 0.96)
    "inverse_masked": 4,           # 1.28  (rows reversed with gaps of 5, row 0; one block alone 1.17, block 14, T 16372; the two (BC, BCx) cases 0.99)
    "fwd_adjoint": 4,              # 1.10  (BC 2, row 0; one block alone 0.89, block 10, T 4096)
    "adjoint": 2,                  # 0.77  (block 14, T 16372)
    "inverse_remix": 2,            # 0.96  (Wiener-EM, mix 0 channel 0; mix-phase 0.95)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("longband_edges_parity", M)
_judge = _T.judge
SHAPES = [(0, 1), (1, 3)]                 # (index into lengths(), BC): S = 3 and S = 5
_ENG = []


@pytest.fixture(scope="module", autouse=True)
def _dump_tables_and_close_the_engine():
    yield
    _T.dump()
    for eng in _ENG:
        eng.close()
    _ENG.clear()


def _engine():
    if not _ENG:
        from xumx_slicq_amd.transforms import SliCQEngine
        _ENG.append(SliCQEngine(edge_plan()[0]))
    return _ENG[0]


def _handle():
    return _engine().handle(torch.device("cuda", torch.cuda.current_device()))


def _enc(x):
    eng = _engine()
    arena, lead, S = eng.forward(x)
    return eng.table.views(arena, lead, S)


def _dec(X, n):
    eng = _engine()
    arena, lead, S = eng.table.as_arena([p.cuda() for p in X])
    return eng.backward(arena, int(np.prod(lead)), S, n).view(*lead, n)


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


def _arena(blocks):
    return torch.cat([b.reshape(-1) for b in blocks]).cuda()


# ---- 1. forward: every band, both shapes ------------------------------------------------------------------------------------------------------
def test_forward_every_band_is_at_fp32_rounding_of_float64():
    from xumx_slicq_amd import _lib
    plan = edge_plan()[1]
    assert int(_lib.lib.xsq_plan_num_long_bands(_handle())) == 16
    bad = []
    for li, BC in SHAPES:
        n = lengths()[li]
        x = audio(n, BC)
        ref = ref64.forward(plan, x)
        e_cpu = flat(ref64.band_rel_err(O.forward(plan, x), ref, True))
        Cd = [c.cpu() for c in _enc(x.cuda())]
        assert len(Cd) == len(BLOCKS) and Cd[0].shape[-3] == (3, 5)[li] and all(bool(torch.isfinite(c).all()) for c in Cd)
        b, _ = _judge("forward", f"n {n} BC {BC}", flat(ref64.band_rel_err(Cd, ref, True)), e_cpu, band_labels(BC), full_table=(BC == 3))
        bad += [f"n {n} BC {BC} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- 2. inverse: one block alone, one band of a block alone, all blocks ---------------------------------------------------------------------------
def test_inverse_of_each_block_alone_is_at_fp32_rounding_of_float64():
    """Coefficients that are zero except in ONE block, for each of the 16 blocks, stacked along a leading dimension (S = 3); then zero
    except in ONE band of a block of several -- f = 1 of 2, f = 2 of 3 -- so that a wrong ``f`` cannot hide in a sum."""
    plan = edge_plan()[1]
    n = lengths()[0]
    bad = []
    for tag, X, labels in (("one block", one_block_rows(3, n), block_labels()),
                           ("one band of a block", one_band_rows(3, n + 1), ["band 6: f 1 of 2, Lg 516", "band 9: f 2 of 3, Lg 1024"])):
        ref = ref64.inverse(plan, X, n)
        e_cpu = ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,))
        y = _dec(X, n).cpu()
        assert y.shape == ref.shape and bool(torch.isfinite(y).all())
        b, _ = _judge("inverse", tag, ref64.rel_err(y, ref, keep=(0,)), e_cpu, labels, full_table=True)
        bad += [f"{tag} {m}" for m in b]
    assert not bad, "\n".join(bad)


def test_inverse_of_all_blocks_is_at_fp32_rounding_of_float64():
    plan = edge_plan()[1]
    bad = []
    for li, BC in SHAPES:
        n = lengths()[li]
        X = random_blocks(BC, (3, 5)[li], n + BC)
        ref = ref64.inverse(plan, X, n)
        y = _dec(X, n).cpu()
        b, _ = _judge("inverse", f"all blocks n {n} BC {BC}", ref64.rel_err(y, ref, keep=(0,)), ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)),
                      [f"row {r}" for r in range(BC)])
        bad += [f"n {n} BC {BC} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- 3. the masked inverse ------------------------------------------------------------------------------------------------------------------------
def _masked(masks, mix, BC, BCx, S, n, out, offs):
    return _engine().backward_masked(_arena(masks), _arena(mix), BC, BCx, S, n, out, offs.cuda())


def test_masked_inverse_is_at_fp32_rounding_of_float64():
    """``backward_masked``: BC = 4 mask channels over BCx = 2 mix channels at S = 3 and BC = 3 over BCx = 1 at S = 5, as
    tests/test_logscale_gpu.py has them; and a mask that is zero except in ONE block, for each block, over one mix channel."""
    plan = edge_plan()[1]
    bad = []
    for li, BC, BCx in ((0, 4, 2), (1, 3, 1)):
        n, S = lengths()[li], (3, 5)[li]
        gen = torch.Generator().manual_seed(n + BC)
        mix = [torch.randn(BCx, F, S, T, 2, generator=gen) for (_, F, T) in BLOCKS]
        masks = [torch.rand(BC, F, S, T, generator=gen) for (_, F, T) in BLOCKS]
        X = [mk[..., None] * mx.repeat(BC // BCx, 1, 1, 1, 1) for mk, mx in zip(masks, mix)]
        ref = ref64.inverse(plan, X, n)
        out = torch.empty(BC, n, dtype=torch.float32, device="cuda")
        _masked(masks, mix, BC, BCx, S, n, out, torch.arange(BC, dtype=torch.int64) * n)
        b, _ = _judge("inverse_masked", f"n {n} BC {BC} BCx {BCx}", ref64.rel_err(out.cpu(), ref, keep=(0,)),
                      ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)), [f"row {r}" for r in range(BC)])
        bad += [f"n {n} BC {BC} BCx {BCx} {m}" for m in b]
    n, S, BC = lengths()[0], 3, len(BLOCKS)
    masks = one_block_rows(S, n + 7, real=True)
    mix = random_blocks(1, S, n + 8)
    X = [mk[..., None] * mx for mk, mx in zip(masks, mix)]
    ref = ref64.inverse(plan, X, n)
    out = torch.empty(BC, n, dtype=torch.float32, device="cuda")
    _masked(masks, mix, BC, 1, S, n, out, torch.arange(BC, dtype=torch.int64) * n)
    b, _ = _judge("inverse_masked", "one block", ref64.rel_err(out.cpu(), ref, keep=(0,)), ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)),
                  block_labels(), full_table=True)
    bad += [f"one block {m}" for m in b]
    assert not bad, "\n".join(bad)


def test_masked_inverse_places_rows_in_reverse_order_with_gaps():
    """``row_offsets`` that are not ``arange(BC) * n``: the rows in reverse order, five samples apart; the gaps keep their fill."""
    plan = edge_plan()[1]
    n, S, BC, BCx, gap, fill = lengths()[0], 3, 4, 2, 5, 7.0
    gen = torch.Generator().manual_seed(n + 11)
    mix = [torch.randn(BCx, F, S, T, 2, generator=gen) for (_, F, T) in BLOCKS]
    masks = [torch.rand(BC, F, S, T, generator=gen) for (_, F, T) in BLOCKS]
    X = [mk[..., None] * mx.repeat(BC // BCx, 1, 1, 1, 1) for mk, mx in zip(masks, mix)]
    ref = ref64.inverse(plan, X, n)
    out = torch.full((BC, n + gap), fill, dtype=torch.float32, device="cuda")
    _masked(masks, mix, BC, BCx, S, n, out, (BC - 1 - torch.arange(BC, dtype=torch.int64)) * (n + gap))
    got = out.cpu()
    assert bool((got[:, n:] == fill).all())
    bad, _ = _judge("inverse_masked", "rows reversed, gaps of 5", ref64.rel_err(got[:, :n].flip(0), ref, keep=(0,)),
                    ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)), [f"row {r}" for r in range(BC)])
    assert not bad, "\n".join(bad)


# ---- 4. both adjoints -------------------------------------------------------------------------------------------------------------------------------
def test_forward_adjoint_is_at_fp32_rounding_of_float64_autograd():
    """S = 3, BC = 2, random cotangents in every block; and cotangents that are zero except in ONE block, for each block.  Reference:
    float64 autograd through ``ref64.forward``; E: the closed form of tests/test_autograd_cpu.py in fp32."""
    plan = edge_plan()[1]
    n, S = lengths()[0], 3
    bad = []
    for tag, G32, labels in (("BC 2", random_blocks(2, S, n + 21), ["row 0", "row 1"]), ("one block", one_block_rows(S, n + 22), block_labels())):
        BC = G32[0].shape[0]
        ref = autograd_forward_adjoint(plan, [g.double() for g in G32], n)
        cpu = forward_adjoint_closed_form(plan, G32, n, dtype=F32)
        got = _engine().forward_adjoint(_arena(G32), (BC,), n)
        assert got.shape == (BC, n) and bool(torch.isfinite(got).all())
        b, _ = _judge("fwd_adjoint", tag, ref64.rel_err(got.cpu(), ref, keep=(0,)), ref64.rel_err(cpu, ref, keep=(0,)), labels, full_table=True)
        bad += [f"{tag} {m}" for m in b]
    assert not bad, "\n".join(bad)


def test_inverse_adjoint_is_at_fp32_rounding_of_float64_autograd():
    """S = 3, BC = 2, per block.  Reference: float64 autograd through ``ref64.inverse``; E: the closed form of tests/test_sdr_cpu.py in
    fp32 over the library's own host window."""
    plan = edge_plan()[1]
    n, S, BC = lengths()[0], 3, 2
    X = [x.double().requires_grad_(True) for x in random_blocks(BC, S, n + 31)]
    gy = torch.randn(BC, n, generator=torch.Generator().manual_seed(n + 32), dtype=F64)
    (ref64.inverse(plan, X, n) * gy).sum().backward()
    ref = [x.grad for x in X]
    gy32 = gy.float()
    cpu = adjoint_closed_form(plan, adjoint_window(plan), gy32, S, dtype=F32)
    eng = _engine()
    got = [v.cpu() for v in eng.table.views(eng.backward_adjoint(gy32.cuda(), S), (BC,), S)]
    bad, _ = _judge("adjoint", f"n {n} BC {BC}", _pair([ref64.rel_err(a, r) for a, r in zip(got, ref)]),
                    _pair([ref64.rel_err(c, r) for c, r in zip(cpu, ref)]), block_labels(), full_table=True)
    assert not bad, "\n".join(bad)


# ---- 5. the remix inverse ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wiener", [False, True])
def test_remix_inverse_is_at_fp32_rounding_of_float64(wiener):
    """``xsq_slicqt_inverse_remix`` on this plan's handle: R = 2 mixes of the four targets, one gain zero in both rows (the target is not
    loaded), one negative; B = 1, S = 3.  Mix-phase (masks + mix) and Wiener-EM (Y).  Each output row against ``ref64.inverse`` of the
    gain-combined coefficients; E: the fp32 oracle on the same coefficients, combined in fp32."""
    from xumx_slicq_amd import _lib
    plan = edge_plan()[1]
    eng = _engine()
    gains = np.asarray([[1.0, 0.0, -0.5, 2.0], [0.25, 0.0, 1.0, -1.0]], dtype=np.float32)
    R, B, S, n = 2, 1, 3, lengths()[0]
    gen = torch.Generator().manual_seed(n + 41 + int(wiener))
    g32 = torch.from_numpy(gains)
    if wiener:
        Y = [torch.randn(4, 2 * B, F, S, T, 2, generator=gen) for (_, F, T) in BLOCKS]
        X64 = [torch.einsum("rt,tc...->rc...", g32.double(), y.double()).reshape(R * 2 * B, *y.shape[2:]) for y in Y]
        X32 = [torch.einsum("rt,tc...->rc...", g32, y).reshape(R * 2 * B, *y.shape[2:]) for y in Y]
        src = (None, None, _arena(Y))
    else:
        mix = [torch.randn(2 * B, F, S, T, 2, generator=gen) for (_, F, T) in BLOCKS]
        masks = [torch.rand(4, 2 * B, F, S, T, generator=gen) for (_, F, T) in BLOCKS]
        X64 = [(torch.einsum("rt,tc...->rc...", g32.double(), mk.double())[..., None] * mx.double()).reshape(R * 2 * B, *mx.shape[1:])
               for mk, mx in zip(masks, mix)]
        X32 = [(torch.einsum("rt,tc...->rc...", g32, mk)[..., None] * mx).reshape(R * 2 * B, *mx.shape[1:]) for mk, mx in zip(masks, mix)]
        src = (_arena(masks), _arena(mix), None)
    ref = ref64.inverse(plan, X64, n)
    h = _handle()
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = eng.workspace(dev, _lib.workspace_bytes("xsq_slicqt_remix_workspace", h, R, B, S, int(wiener)))
    out = torch.empty(R * 2 * B, n, dtype=torch.float32, device="cuda")
    ptr = [t.data_ptr() if t is not None else None for t in src]
    _lib.call("xsq_slicqt_inverse_remix", h, ptr[0], ptr[1], ptr[2], gains.ctypes.data_as(C.c_void_p), R, B, S, n, out.data_ptr(), None,
              ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    got = out.cpu()
    assert bool(torch.isfinite(got).all())
    bad, _ = _judge("inverse_remix", "Wiener-EM (Y)" if wiener else "mix-phase (masks, mix)", ref64.rel_err(got, ref, keep=(0,)),
                    ref64.rel_err(O.inverse(plan, X32, n), ref, keep=(0,)), [f"mix {r} channel {c}" for r in range(R) for c in range(2 * B)])
    assert not bad, "\n".join(bad)


# ---- 6. the same bits again, and on another stream ------------------------------------------------------------------------------------------------
def test_second_call_and_non_default_stream_give_the_same_bits():
    """The engine parks its sub-transforms on its own output row and sums in a fixed order."""
    n = lengths()[1]
    x = audio(n, 3).cuda()
    C1 = [c.clone() for c in _enc(x)]
    y1 = _dec(C1, n).clone()
    C2 = _enc(x)
    assert all(torch.equal(a, b) for a, b in zip(C1, C2)) and torch.equal(_dec(C2, n), y1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        C3 = _enc(x)
        y3 = _dec(C3, n)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(C1, C3)) and torch.equal(y3, y1)
