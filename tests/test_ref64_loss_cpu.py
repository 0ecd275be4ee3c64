"""Host side of tests/test_ref64_loss_gpu.py: the float64 restatements of the loss terms per block and of the statistics sums per
bin (``ref64.block_losses``, ``ref64.magnitude_sums``) pinned to what is already pinned to the reference, the index arithmetic of
the loss kernel's mask walk over the block tables the GPU tests use, the unit phase of the mix-phase kernel in fp32 on the host, and
the argument checks of the three C entry points (no device needed: they return before any HIP call)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64
from xumx_slicq_amd.synth import synth_audio

XSQ_ERR_ARG = -1
F32, F64 = torch.float32, torch.float64


# ---- loss terms per block ------------------------------------------------------------------------------------------------------
def _random_lists(shapes, B, S, seed):
    gen = torch.Generator().manual_seed(seed)
    pred = [torch.randn(4, B, 2, F, S, T, 2, generator=gen) for F, T in shapes]
    targ = [torch.randn(4, B, 2, F, S, T, 2, generator=gen) for F, T in shapes]
    msks = [torch.rand(4, B, 2, F, S, T, generator=gen) for F, T in shapes]
    return pred, targ, msks


def test_block_mean_of_the_fp32_arm_is_the_oracle_loss():
    from oracle import loss as oloss
    pred, targ, msks = _random_lists([(3, 16), (1, 28), (2, 40), (3, 7), (1, 1)], 2, 5, seed=0)
    per_block = ref64.block_losses(pred, targ, msks, F32)
    assert per_block.shape == (5, 2) and per_block.dtype == np.float64
    a, b = float(oloss.complex_mse(pred, targ)), float(oloss.mask_sum(msks))
    assert abs(per_block[:, 0].mean() - a) < 1e-5 * a
    assert abs(per_block[:, 1].mean() - b) < 1e-5 * b
    # without masks the first column is the same and the second is zero
    alone = ref64.block_losses(pred, targ, None, F32)
    assert np.array_equal(alone[:, 0], per_block[:, 0]) and not alone[:, 1].any()
    # the float64 arm is another number, at fp32 rounding of the fp32 one, block by block
    ref = ref64.block_losses(pred, targ, msks, F64)
    rel = np.abs(per_block - ref) / ref
    print("fp32 arm vs float64 arm, per block:", rel)
    assert (rel > 0).all() and (rel < 1e-6).all()


def test_block_mean_of_the_fp32_arm_is_the_reference_validation_step(oracle_plan, seeded_sd):
    """The blocks of ``oloss.validation_step``'s own estimates, targets and masks: the mean over the 70 blocks of the fp32 arm is
    the reference's (mse, mask) of tests/golden/validation_step.npz, at the tolerances tests/test_loss.py holds the oracle to."""
    from oracle import slicqt as oslicqt
    g = load_golden("validation_step.npz")
    n = int(g["n"])
    y_t = torch.stack([0.5 * synth_audio(n, seed=500 + j, nb_samples=2) for j in range(4)])
    with torch.no_grad():
        Y, masks = omodel.unmix(seeded_sd, oslicqt.forward(oracle_plan, y_t.sum(0)), causal=False, wiener=True)
        Yt = oslicqt.forward(oracle_plan, y_t)
    per_block = ref64.block_losses(Y, Yt, masks, F32)
    assert per_block.shape == (70, 2)
    mse, msk = per_block.mean(0)
    assert abs(mse - float(g["mse"])) < 1e-5 * float(g["mse"]) + 1e-7
    assert abs(msk - float(g["mask"])) < 1e-5 * float(g["mask"]) + 1e-7
    ref = ref64.block_losses(Y, Yt, masks, F64)
    rel = np.abs(per_block - ref) / ref
    assert rel.max() > 0 and (rel < 1e-6).all(), rel.max()


# ---- statistics sums per bin ---------------------------------------------------------------------------------------------------
def test_magnitude_sums_through_the_host_formula_are_the_reference_statistics(oracle_plan):
    from oracle import slicqt as oslicqt
    g = load_golden("statistics.npz")
    tracks = [synth_audio(int(n), seed=900 + i)[0] for i, n in enumerate(g["lens"])]
    acc = {F32: None, F64: None}
    frames = np.zeros(len(oracle_plan.blocks))
    worst = 0.0
    for x in tracks:
        X = oslicqt.forward(oracle_plan, x[None])                   # list of (1, C, F, S, T, 2)
        frames += [Xb.shape[-3] * Xb.shape[-2] for Xb in X]
        sums = {dt: ref64.magnitude_sums(X, dt) for dt in acc}
        assert [s.shape for s in sums[F64]] == [(F, 2) for (_, F, _) in oracle_plan.blocks]
        rel = np.concatenate([np.abs(a - b) / b for a, b in zip(sums[F32], sums[F64])])
        assert (rel < 1e-6).all(), rel.max()
        worst = max(worst, float(rel.max()))
        for dt in acc:
            acc[dt] = sums[dt] if acc[dt] is None else [a + s for a, s in zip(acc[dt], sums[dt])]
    assert worst > 0                                                 # (the two arms are not the same arithmetic)
    for dt in acc:
        means, stds = ref64.statistics_from_sums(acc[dt], frames)
        assert np.allclose(np.concatenate(means), g["means"], rtol=1e-5, atol=1e-6)
        assert np.allclose(np.concatenate(stds), g["stds"], rtol=1e-5, atol=1e-6)


def test_magnitude_sums_of_exact_magnitudes_are_exact():
    """(3, 4) * 2^k has magnitude 5 * 2^k in every arithmetic: both arms give the integer sums (the GPU probe test relies on it)."""
    X = torch.zeros(4, 2, 3, 5, 2)
    X[1, 0, 0, 0] = torch.tensor([3.0, 4.0]) * 4
    X[2, 0, 2, 4] = torch.tensor([-4.0, 3.0]) * 8
    X[0, 1, 1, 1] = torch.tensor([3.0, -4.0])
    for dt in (F32, F64):
        (s,) = ref64.magnitude_sums([X], dt)
        assert np.array_equal(s, [[5.0 + 10.0, 25.0 + 100.0], [1.25, 1.25 ** 2]])


# ---- the loss kernel's walk of the mask arena, restated on the host --------------------------------------------------------------
def _mask_accesses(shapes, B, S, halves):
    """Every vector access (float offset, width in floats, block, target) of k_loss_partial to the real arena for one block table,
    from the work table of csrc/loss.hip: quads i = 0, 4, .. below nreal * 2 / 4 * 4 guarded by i < nreal; a table with any
    nreal % 4 != 0 (``halves``) takes two float2 accesses per quad, each guarded by k < nreal."""
    out, cum = [], 0
    for b, (F, T) in enumerate(shapes):
        nreal = B * 2 * F * S * T
        base_r = B * 8 * S * cum
        for i in range(0, 2 * nreal, 4):
            for j in range(4):
                if halves:
                    out += [(base_r + j * nreal + k, 2, b, j) for k in (i, i + 2) if k < nreal]
                elif i < nreal:
                    out.append((base_r + j * nreal + i, 4, b, j))
        cum += F * T
    return out


LISTS = [[(1, 3, 5, 7), (1, 1, 5, 1), (1, 2, 5, 16)], [(1, 2, 5, 16), (1, 3, 5, 7)], [(1, 1, 1, 1)], [(3, 5, 3, 9), (3, 1, 3, 28)],
         [(2, 3, 5, 16), (2, 1, 5, 28), (2, 2, 5, 40)]]


@pytest.mark.parametrize("blocks", LISTS)
def test_mask_walk_stays_inside_its_sub_arena_and_aligned(blocks):
    """The lists of the GPU tests.  With the float2 arm for tables that have an odd B F S T: every access inside the (block, target)
    sub-arena it belongs to, aligned to its own width, every float read once.  With the float4 walk alone (the kernel before this
    arm existed) the odd tables read past their sub-arena -- for the last block's last target past the arena -- and at 8-byte
    alignment: the defect the arm closes, e.g. (1, 3, 5, 7): nreal = 210, the quad at 208 reads floats 208 .. 211."""
    B, S = blocks[0][0], blocks[0][2]
    shapes = [(F, T) for (_, F, _, T) in blocks]
    nreal = [B * 2 * F * S * T for F, T in shapes]
    odd = any(n % 4 for n in nreal)
    total = 4 * sum(nreal)
    start = np.concatenate([[0], np.cumsum([4 * n for n in nreal])])
    seen = np.zeros(total, dtype=np.int64)
    for off, width, b, j in _mask_accesses(shapes, B, S, halves=odd):
        lo = start[b] + j * nreal[b]
        assert lo <= off and off + width <= lo + nreal[b], (off, width, b, j)
        assert off % width == 0, (off, width, b, j)
        seen[off:off + width] += 1
    assert (seen == 1).all()
    if odd:
        bad = [(off, b, j) for off, width, b, j in _mask_accesses(shapes, B, S, halves=False)
               if off + width > start[b] + (j + 1) * nreal[b] or off % 4]
        assert bad
        assert (max(off + 4 for off, _, _ in bad) > total) == (nreal[-1] % 4 != 0)


def test_plan_tables_keep_the_float4_walk(oracle_plan):
    for B in (1, 2, 3):
        for S in (1, 3, 5):
            assert all((B * 2 * F * S * T) % 4 == 0 for (_, F, T) in oracle_plan.blocks)


# ---- the mix-phase kernel's unit phase, restated on the host in fp32 ---------------------------------------------------------------
def _unit_phase_fp32(x, scaled=True):
    """unit_phase of csrc/wiener.hip in numpy float32; ``scaled=False``: the expression the kernel had before."""
    x = x.astype(np.float32)
    tiny, big = np.finfo(np.float32).tiny, np.finfo(np.float32).max
    with np.errstate(all="ignore"):
        a2 = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]
        ax = np.sqrt(a2)
        plain = np.where((ax > 0)[..., None], x / ax[..., None], np.float32([1, 0]))
        if not scaled:
            return plain.astype(np.float32)
        s = np.maximum(np.abs(x[..., 0]), np.abs(x[..., 1]))
        y = x / s[..., None]
        y = y / np.sqrt(y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1])[..., None]
        y = np.where((s > 0)[..., None], y, np.float32([1, 0]))
        return np.where(((a2 >= tiny) & (a2 <= big))[..., None], plain, y).astype(np.float32)


@pytest.mark.parametrize("lo,hi,old_fails", [(-30, -19, True), (19, 30, True), (-3, 3, False)])
def test_unit_phase_of_tiny_and_huge_mix_values(lo, hi, old_fails):
    """The scaled form is at fp32 rounding of ref64.phasemix_sep for moduli 1e-30 .. 1e30; the plain form the kernel had is wrong
    by order one below 1e-19 (re^2 + im^2 underflows: angle 0) and above 1.8e19 (it overflows: output 0)."""
    rng = np.random.default_rng(7)
    mod = 10.0 ** rng.uniform(lo, hi, 4096)
    ph = rng.uniform(-np.pi, np.pi, 4096)
    x = np.stack((mod * np.cos(ph), mod * np.sin(ph)), -1).astype(np.float32)
    X = torch.from_numpy(x).reshape(1, 2, 1, 1, 2048, 2)
    ref = ref64.phasemix_sep(X, torch.ones(4, 1, 2, 1, 1, 2048))[0]
    new = float(ref64.rel_err(torch.from_numpy(_unit_phase_fp32(x)).reshape(ref.shape), ref)[1])
    old = float(ref64.rel_err(torch.from_numpy(_unit_phase_fp32(x, scaled=False)).reshape(ref.shape), ref)[1])
    print(f"moduli 1e{lo} .. 1e{hi}: scaled form {new:.3e}, plain form {old:.3e}")
    assert new < 4e-7
    assert (old > 0.5) == old_fails
    if not old_fails:                                     # where the sum of squares is a normal number the bits are the old ones
        assert np.array_equal(_unit_phase_fp32(x), _unit_phase_fp32(x, scaled=False))
    assert np.array_equal(_unit_phase_fp32(np.zeros((3, 2))), np.float32([[1, 0]] * 3))
    assert np.array_equal(_unit_phase_fp32(np.float32([[1e-30, 1e-30]]), scaled=False), np.float32([[1, 0]]))      # the issue's example


# ---- argument checks of the C entry points ---------------------------------------------------------------------------------------
def test_loss_and_statistics_entry_points_check_their_arguments_without_a_device():
    """Null pointers, B, S or C <= 0 and a workspace that is too small are XSQ_ERR_ARG before any HIP call (the pointers are never
    followed: a dummy host buffer stands for all of them); the workspace query returns 0 on bad arguments."""
    from xumx_slicq_amd import _lib
    L = _lib.lib
    F, T = np.asarray([3, 1], dtype=np.int32), np.asarray([7, 16], dtype=np.int32)
    f, t = F.ctypes.data, T.ctypes.data
    buf = np.zeros(64, dtype=np.float64)
    p, big = buf.ctypes.data, 1 << 40
    need = L.xsq_loss_workspace(2, f, t, 2, 5)
    assert need > 0
    for bad in ((0, f, t, 2, 5), (-1, f, t, 2, 5), (2, None, t, 2, 5), (2, f, None, 2, 5), (2, f, t, 0, 5), (2, f, t, 2, 0), (2, f, t, -1, 5)):
        assert L.xsq_loss_workspace(*bad) == 0, bad
    ok = dict(n=2, F=f, T=t, pred=p, target=p, masks=p, B=2, S=5, out=p, ws=p, ws_bytes=big)
    for change, word in ((dict(pred=None), "null"), (dict(target=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"),
                         (dict(F=None), "null"), (dict(T=None), "null"), (dict(n=0), "null"), (dict(B=0), "B="), (dict(B=-2), "B="),
                         (dict(S=0), "S="), (dict(S=-1), "S="), (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace")):
        a = dict(ok, **change)
        rc = L.xsq_loss_forward(a["n"], a["F"], a["T"], a["pred"], a["target"], a["masks"], a["B"], a["S"], a["out"], a["ws"], a["ws_bytes"], None)
        assert rc == XSQ_ERR_ARG and word in _lib.last_error(), (change, rc, _lib.last_error())
    ok = dict(n=2, F=f, T=t, X=p, C=2, S=5, out=p, ws=p, ws_bytes=big)
    rows = int(F.sum())
    for change, word in ((dict(X=None), "null"), (dict(out=None), "null"), (dict(ws=None), "null"), (dict(F=None), "null"),
                         (dict(T=None), "null"), (dict(n=0), "null"), (dict(C=0), "C="), (dict(C=-1), "C="), (dict(S=0), "S="),
                         (dict(S=-3), "S="), (dict(ws_bytes=32 * rows - 1), "workspace"), (dict(ws_bytes=0), "workspace")):
        a = dict(ok, **change)
        rc = L.xsq_magnitude_stats(a["n"], a["F"], a["T"], a["X"], a["C"], a["S"], a["out"], a["ws"], a["ws_bytes"], None)
        assert rc == XSQ_ERR_ARG and word in _lib.last_error(), (change, rc, _lib.last_error())
