"""The loss terms per block (k_loss_partial / k_loss_combine), the dataset statistics per bin (k_magnitude_stats) and the mix-phase
estimate (k_phasemix) at fp32 rounding of the float64 reference (oracle/ref64.py: block_losses, magnitude_sums, phasemix_sep).

Metric and rule are the ones of tests/test_ref64_gpu.py: ``ref64.rel_err`` per block, bin or class; e_gpu = the kernels against the
float64 arm, e_cpu = the fp32 CPU oracle (the fp32 arm of the same helper, ``omodel.phasemix_sep`` in fp32) against it on the same
input; assert  e_gpu <= M * E,  E the LARGEST e_cpu over the members of the stage on that input; M per stage by the rule of
oracle/parity.py.  Beside the random inputs every kernel gets a PROBE input whose result is exact in fp32 and in fp64 (errors and
magnitudes that are powers of two at the first and last element of every sub-arena and at the seams of the work items): a dropped,
doubled or misplaced element moves a block by at least 1 / 256 of its value and the comparison is to fp64 rounding.

Two defects were found by reading the kernels for these tests and are fixed with them (the host-side evidence is in
tests/test_ref64_loss_cpu.py): the float4 walk of the mask arena over-read every target whose B F S T is odd
(``test_lists_outside_the_plan``: the mask term of (1, 3, 5, 7) was off by about 2 / 210 of its value, the probe doubles), and the
mix-phase kernel lost the phase of mix values below 1e-19 and above 1.8e19 (``test_mixphase``: classes tiny and huge).
"""
import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import ref64
from oracle.parity import M_CAP, Tables
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
EXACT = 8 * 2.0 ** -52          # probe inputs: every partial sum is exact, at most two fp64 roundings on each side (1 / n and the product)

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_loss.json): the
# smallest power of two that is at least twice that ratio
M = {
    "loss/mse": 1,                 # 0.33  (lists outside the plan: list 2 block 0, (1, 1, 1, 1)); plan arena 0.03 (block 14)
    "loss/mask": 1,                # 0.17  (lists outside the plan: list 0 block 1, (1, 1, 5, 1)); plan arena 0.05 (block 36)
    "stats": 8,                    # 2.35  (table S = 1, C = 3: block 0 bin 2, sumsq of 7 frames; E is 2.9e-8 there); Bark-262 1.16
    "phasemix": 2,                 # 0.97  ((1, 1, 1, 1), class normal); tiny 0.75, huge below
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())

_T = Tables("ref64_loss", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


@pytest.fixture(scope="module")
def fb():
    from xumx_slicq_amd.transforms import NSGTBase, make_filterbanks
    base = NSGTBase("bark", 262, 32.9, device="cuda")
    enc, dec = make_filterbanks(base)
    return base, enc, dec


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def _gpu_losses(pred, target, masks):
    from xumx_slicq_amd.loss import _per_block_losses
    up = lambda ts: None if ts is None else [t.cuda() for t in ts]
    return _per_block_losses(up(pred), up(target), up(masks)).cpu().numpy()


def _gpu_stats(shapes, X_list, C, S):
    """xsq_magnitude_stats on blocks (C, F_b, S, T_b, 2) laid out back to back, as xumx_slicq_amd/statistics.py calls it:
    (sum_b F_b, 2) float64."""
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.arena import BlockTable
    from xumx_slicq_amd.phase import _tables, _workspace
    table = BlockTable(shapes)
    F, T = _tables(table)
    assert [tuple(x.shape) for x in X_list] == [(C, f, S, t, 2) for f, t in shapes]
    arena = torch.cat([x.reshape(-1) for x in X_list]).float().cuda()
    rows = int(F.sum())
    with torch.cuda.device(arena.device):
        out = torch.empty(rows, 2, dtype=F64, device=arena.device)
        ws = _workspace(arena.device, 32 * rows)
        _lib.check(_lib.lib.xsq_magnitude_stats(len(table), F.ctypes.data, T.ctypes.data, arena.data_ptr(), C, S, out.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "xsq_magnitude_stats")
    return out.cpu().numpy()


def _gpu_phasemix(X, mag):
    from xumx_slicq_amd.phase import blockwise_phasemix_sep
    Xd, magd = X.cuda(), mag.cuda()
    X0, mag0 = Xd.clone(), magd.clone()
    Y = blockwise_phasemix_sep(Xd, magd)
    assert torch.equal(Xd, X0) and torch.equal(magd, mag0)          # the inputs are not modified
    return Y.cpu()


# ---- judge -------------------------------------------------------------------------------------------------------------------------
def _scalar_err(got, ref):
    """``ref64.rel_err`` of every scalar of a vector on its own (|got - ref| / |ref|; a zero reference raises)."""
    got, ref = (torch.as_tensor(np.asarray(a, dtype=np.float64)).reshape(-1, 1) for a in (got, ref))
    return ref64.rel_err(got, ref, keep=(0,))


def _judge_losses(case, got, r64, r32, labels, masks=True):
    bad = []
    for col, stage in ((0, "loss/mse"), (1, "loss/mask"))[:2 if masks else 1]:
        b, _ = _T.judge(stage, case, _scalar_err(got[:, col], r64[:, col]), _scalar_err(r32[:, col], r64[:, col]), labels, full_table=True)
        bad += [f"{stage} {case} {m}" for m in b]
    return bad


def _assert_exact(case, got, ref, labels):
    rel = np.abs(got - ref) / ref
    print(f"\n[probe] {case}: worst |gpu - float64| / float64 = {rel.max():.3e} (allowed {EXACT:.3e})")
    bad = [f"{case} {labels[b]} {('mse', 'mask')[c]}: gpu {got[b, c]!r} float64 {ref[b, c]!r}" for b, c in zip(*np.nonzero(~(rel <= EXACT)))]
    assert not bad, "\n".join(bad[:40])


# ---- loss inputs -------------------------------------------------------------------------------------------------------------------
def _noisy(target, seed):
    """pred = target + noise, masks: the noise amplitude 10^(-2 .. 1) is drawn per (block, target) -- a mix-up of blocks or targets
    changes a value by orders of magnitude -- and the masks are uniform in (0, 1) plus an offset per (block, target)."""
    gen = torch.Generator().manual_seed(seed)
    pred, masks = [], []
    for t in target:
        amp = 10.0 ** (3.0 * torch.rand(4, generator=gen) - 2.0)
        off = 0.25 * torch.randperm(4, generator=gen).float()
        shape = (4,) + (1,) * (t.dim() - 1)
        pred.append(t + amp.view(shape) * torch.randn(t.shape, generator=gen))
        masks.append(torch.rand(t.shape[:-1], generator=gen) + off.view(shape[:-1]))
    return pred, masks


SEAM = 4 * 4096                 # floats of one work item of k_loss_partial


def _probes(target):
    """(pred, target', masks): pred == target' except at the probe floats of every (block, target) sub-arena -- the first, the last,
    and SEAM - 1 and SEAM where the sub-arena is longer -- where target' is 0 and pred is 2^k, k = 4 * position + target (probes of
    the four targets at one position share a quad: adjacent k keep the fp32 sum of their squares exact).  Masks are 0.25 (the four
    sum to exactly 1) except at the first and last float of every real sub-arena: 0.25 + 2^k."""
    pred, targ, masks = [], [], []
    for t in target:
        t = t.clone()
        p = t.clone()
        m = torch.full(t.shape[:-1], 0.25)
        nc = t[0].numel()
        where_c = sorted({0, nc - 1} | ({SEAM - 1, SEAM} if nc > SEAM + 1 else set()))
        where_r = sorted({0, nc // 2 - 1})
        for j in range(4):
            for k, i in enumerate(where_c):
                t[j].view(-1)[i] = 0.0
                p[j].view(-1)[i] = 2.0 ** (4 * k + j)
            for k, i in enumerate(where_r):
                m[j].view(-1)[i] = 0.25 + 2.0 ** (4 * k + j)
        pred.append(p), targ.append(t), masks.append(m)
    return pred, targ, masks


# ---- loss: the plan arena ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_targets(fb):
    """The GPU sliCQT of four synth stems, B = 2, n = 9031 (S = 3): all 70 blocks of Bark-262 as (4, 2, 2, F, 3, T, 2) on the host --
    blocks of one partial work item (F = 1, T = 16: 192 quads) and of several (F = 86, T = 16: 16,512 quads, a seam at SEAM)."""
    base, enc, dec = fb
    y_t = torch.stack([0.5 * synth_audio(9031, seed=700 + j, nb_samples=2) for j in range(4)])
    Yt = [c.cpu() for c in enc(y_t.cuda())]
    assert len(Yt) == 70 and Yt[1].shape == (4, 2, 2, 86, 3, 16, 2)
    assert min(t[0].numel() for t in Yt) < SEAM < max(t[0].numel() for t in Yt)
    return Yt


def _block_labels(blocks):
    return [f"block {b} {tuple(t.shape[1:-1])}" for b, t in enumerate(blocks)]


def test_plan_arena_every_block_of_both_terms(plan_targets):
    Yt = plan_targets
    pred, masks = _noisy(Yt, seed=1)
    got = _gpu_losses(pred, Yt, masks)
    assert got.shape == (70, 2)
    r64, r32 = ref64.block_losses(pred, Yt, masks, F64), ref64.block_losses(pred, Yt, masks, F32)
    bad = _judge_losses("Bark-262 B=2 n=9031", got, r64, r32, _block_labels(Yt))
    assert not bad, "\n".join(bad)
    # without masks: the complex-MSE column bit for bit, the mask column zero
    alone = _gpu_losses(pred, Yt, None)
    assert np.array_equal(alone[:, 0], got[:, 0]) and not alone[:, 1].any()


def test_plan_arena_probes(plan_targets):
    pred, targ, masks = _probes(plan_targets)
    assert sum(int((p != t).sum()) for p, t in zip(pred, targ)) == 4 * (2 * 70 + 2 * sum(t[0].numel() > SEAM + 1 for t in targ))
    got = _gpu_losses(pred, targ, masks)
    _assert_exact("Bark-262 B=2 n=9031", got, ref64.block_losses(pred, targ, masks, F64), _block_labels(targ))


# ---- loss: block lists outside the plan ----------------------------------------------------------------------------------------------
LISTS = [[(1, 3, 5, 7), (1, 1, 5, 1), (1, 2, 5, 16)],       # B F S T odd, odd, then even last: the float2 arm of the mask walk
         [(1, 2, 5, 16), (1, 3, 5, 7)],                     # odd last: the float4 walk read past the arena
         [(1, 1, 1, 1)],                                    # nreal = 2: one quad of the complex arena, half a quad of masks
         [(3, 5, 3, 9), (3, 1, 3, 28)],
         [(2, 3, 5, 16), (2, 1, 5, 28), (2, 2, 5, 40)]]     # the even shapes of tests/test_loss.py: the float4 walk


def test_lists_outside_the_plan():
    """Every list through ``_per_block_losses`` (judged per block: all lists are members of one table per stage) and through the two
    criteria, which must return the fp32 rounding of the mean of those blocks; then the probe input of every list."""
    from xumx_slicq_amd.loss import ComplexMSELossCriterion, MaskSumLossCriterion
    gen = torch.Generator().manual_seed(2)
    got, r64, r32, labels = [], [], [], []
    for k, blocks in enumerate(LISTS):
        targ = [torch.randn(4, B, 2, F, S, T, 2, generator=gen) for (B, F, S, T) in blocks]
        pred, masks = _noisy(targ, seed=10 + k)
        g = _gpu_losses(pred, targ, masks)
        assert g.shape == (len(blocks), 2)
        got.append(g), r64.append(ref64.block_losses(pred, targ, masks, F64)), r32.append(ref64.block_losses(pred, targ, masks, F32))
        labels += [f"list {k} block {b} {s}" for b, s in enumerate(blocks)]
        a = ComplexMSELossCriterion()([p.cuda() for p in pred], [t.cuda() for t in targ])
        m = MaskSumLossCriterion()([m.cuda() for m in masks])
        assert a.dtype == m.dtype == F32
        assert float(a) == float(torch.from_numpy(g[:, 0]).mean().float()) and float(m) == float(torch.from_numpy(g[:, 1]).mean().float())
        pp, pt, pm = _probes(targ)
        _assert_exact(f"list {k}", _gpu_losses(pp, pt, pm), ref64.block_losses(pp, pt, pm, F64), [str(s) for s in blocks])
    bad = _judge_losses("lists outside the plan", *(np.concatenate(a) for a in (got, r64, r32)), labels)
    assert not bad, "\n".join(bad)


# ---- statistics: the kernel ----------------------------------------------------------------------------------------------------------
STAT_TABLE = [(3, 7), (1, 1), (2, 256), (1, 257), (4, 300)]      # (F, T): with S = 1 rows of 7, 1, 256, 257 and 300 frames (one pass of 256 lanes, two)


def _stat_labels(shapes):
    return [f"block {b} bin {f} {q}" for b, (F, _) in enumerate(shapes) for f in range(F) for q in ("sum", "sumsq")]


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("S", [1, 5])
def test_statistics_kernel_every_bin(S, C):
    """Complex Gaussian input, scale 10^(-3 .. 2) drawn per (block, bin): sum and sum of squares of every bin against the float64 arm."""
    gen = torch.Generator().manual_seed(100 * S + C)
    X = [torch.randn(C, F, S, T, 2, generator=gen) * (10.0 ** (5.0 * torch.rand(F, generator=gen) - 3.0)).view(1, F, 1, 1, 1) for F, T in STAT_TABLE]
    got = _gpu_stats(STAT_TABLE, X, C, S)
    r64, r32 = (np.concatenate(ref64.magnitude_sums(X, dt)) for dt in (F64, F32))
    assert got.shape == r64.shape == (11, 2)
    bad, _ = _T.judge("stats", f"table S={S} C={C}", _scalar_err(got, r64), _scalar_err(r32, r64), _stat_labels(STAT_TABLE), full_table=True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("S", [1, 5])
def test_statistics_kernel_probes(S, C):
    """All zero except (3, 4) * 2^k at frames 0, 255, 256 and N - 1 of every bin (where they exist), in one channel: the magnitudes
    5 * 2^k, their channel means and every sum are exact -- the kernel must equal the float64 arm."""
    X, row = [], 0
    for F, T in STAT_TABLE:
        x = torch.zeros(C, F, S * T, 2)
        for f in range(F):
            for i, n in enumerate(sorted({0, 255, 256, S * T - 1} & set(range(S * T)))):
                x[(row + i) % C, f, n] = torch.tensor([3.0, 4.0]) * 2.0 ** ((row + 3 * i) % 8)
            row += 1
        X.append(x.reshape(C, F, S, T, 2))
    ref = np.concatenate(ref64.magnitude_sums(X, F64))
    assert (ref > 0).all()
    assert np.array_equal(_gpu_stats(STAT_TABLE, X, C, S), ref)


# ---- statistics: the plan ------------------------------------------------------------------------------------------------------------
def test_statistics_of_the_plan_every_bin_and_the_merged_means(fb, oracle_plan):
    """Bark-262, a mono track of 9,031 samples and a stereo one of 30,000.  The coefficients are the GPU encoder's own (it is
    deterministic: ``get_statistics`` below computes the same ones), so only the statistics kernel is judged: all 263 bins of each
    track against the float64 arm.  Then ``get_statistics`` over both tracks against the host formula (``ref64.statistics_from_sums``)
    on the kernel's own float64 sums merged over the tracks: the same fp64 arithmetic, 1e-12 relative -- and, since a mean is a sum
    over a count, the merged means against the merged sums of the float64 arm under the bound of the sums."""
    from xumx_slicq_amd.statistics import get_statistics
    base, enc, dec = fb
    eng = base.nsgt
    shapes = eng.table.shapes
    assert shapes == [(F, T) for (_, F, T) in oracle_plan.blocks]
    tracks = [synth_audio(9031, seed=910)[0][:1], synth_audio(30000, seed=911)[0]]
    assert [tuple(t.shape) for t in tracks] == [(1, 9031), (2, 30000)]
    labels = _stat_labels(shapes)
    merged = {k: [np.zeros((F, 2)) for F, _ in shapes] for k in ("gpu", "r64", "r32")}
    frames = np.zeros(len(shapes))
    bad = []
    for x in tracks:
        arena, lead, S = eng.forward(x[None].cuda())
        C = lead[-1]
        X = [v[0].cpu() for v in eng.table.views(arena, lead, S)]
        assert C == x.shape[0] and S == oracle_plan.nslices(x.shape[-1])
        got = _gpu_stats(shapes, X, C, S)
        r64, r32 = ref64.magnitude_sums(X, F64), ref64.magnitude_sums(X, F32)
        assert got.shape == (263, 2)
        b, _ = _T.judge("stats", f"Bark-262 n={x.shape[-1]} C={C}", _scalar_err(got, np.concatenate(r64)),
                        _scalar_err(np.concatenate(r32), np.concatenate(r64)), labels, full_table=True)
        bad += b
        o = 0
        for k, (F, T) in enumerate(shapes):
            merged["gpu"][k] += got[o:o + F]
            merged["r64"][k] += r64[k]
            merged["r32"][k] += r32[k]
            o += F
        frames += [S * T for _, T in shapes]
    assert not bad, "\n".join(bad)
    means, stds = get_statistics((enc, dec, None), [t.cuda() for t in tracks])
    want_means, want_stds = ref64.statistics_from_sums(merged["gpu"], frames)
    for name, a, w in (("means", means, want_means), ("stds", stds, want_stds)):
        a, w = np.concatenate(a), np.concatenate(w)
        assert a.shape == (263,) and (np.abs(a - w) <= 1e-12 * np.abs(w)).all(), (name, np.abs(a / w - 1).max())
    m64, _ = ref64.statistics_from_sums(merged["r64"], frames)
    m32, _ = ref64.statistics_from_sums(merged["r32"], frames)
    b, _ = _T.judge("stats", "Bark-262 merged means", _scalar_err(np.concatenate(means), np.concatenate(m64)),
                    _scalar_err(np.concatenate(m32), np.concatenate(m64)), [f"block {b} bin {f}" for b, (F, _) in enumerate(shapes) for f in range(F)], full_table=True)
    assert not b, "\n".join(b)


# ---- mix-phase -----------------------------------------------------------------------------------------------------------------------
def _mix_values(cls, n, gen):
    """n complex mix values of one class as (n, 2) fp32."""
    if cls == "normal":
        return torch.randn(n, 2, generator=gen)
    if cls == "zero":
        return torch.zeros(n, 2)                                      # +0 in both parts (-0: oracle and reference disagree, quirk A2)
    lo, hi = {"tiny": (-30.0, -19.0), "huge": (19.0, 30.0)}[cls]
    mod = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, dtype=F64))
    ph = (2.0 * torch.rand(n, generator=gen, dtype=F64) - 1.0) * np.pi
    return torch.stack((mod * torch.cos(ph), mod * torch.sin(ph)), dim=-1).float()


CLASSES = ("normal", "zero", "tiny", "huge")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 26, 2, 100)])
def test_mixphase(shape):
    """``blockwise_phasemix_sep`` with Gaussian magnitudes (negative ones too) and mix values in labelled classes: one input per
    class (the smallest shape has two mix values) and, where there are enough, one with the classes interleaved; ``rel_err`` per
    class against ``ref64.phasemix_sep``, E from ``omodel.phasemix_sep`` in fp32 over the members of the table.  The zero class has no
    error to scale (angle(0) = 0 is exact everywhere): there Y == (mag, 0), bit for bit."""
    B, F, S, T = shape
    n = B * 2 * F * S * T
    gen = torch.Generator().manual_seed(n)
    inputs = [(c, _mix_values(c, n, gen), [c] * n) for c in CLASSES]
    if n >= 8:
        lab = [CLASSES[int(i)] for i in torch.randint(0, 4, (n,), generator=gen)]
        x = torch.stack([_mix_values(c, 1, gen)[0] for c in lab])
        inputs.append(("mixed", x, lab))
    labels, e_gpu, e_cpu = [], [], []
    for name, x, lab in inputs:
        X = x.reshape(B, 2, F, S, T, 2)
        mag = torch.randn(4, B, 2, F, S, T, generator=gen)
        Y = _gpu_phasemix(X, mag)
        assert Y.shape == (4, B, 2, F, S, T, 2) and Y.dtype == F32
        ref, cpu = ref64.phasemix_sep(X, mag), omodel.phasemix_sep(X, mag)
        for c in sorted(set(lab)):
            sel = torch.tensor([l == c for l in lab])
            pick = lambda t: t.reshape(4, n, 2)[:, sel]
            if c == "zero":
                assert torch.equal(pick(Y), torch.stack((mag.reshape(4, n)[:, sel], torch.zeros(4, int(sel.sum()))), dim=-1)), name
                assert torch.equal(pick(Y).double(), pick(ref))
                continue
            labels.append(f"{name}/{c}" if name == "mixed" else c)
            e_gpu.append(ref64.rel_err(pick(Y), pick(ref)))
            e_cpu.append(ref64.rel_err(pick(cpu), pick(ref)))
    bad, _ = _T.judge("phasemix", f"(B, F, S, T) = {shape}", tuple(zip(*e_gpu)), tuple(zip(*e_cpu)), labels, full_table=True)
    assert not bad, "\n".join(bad)
