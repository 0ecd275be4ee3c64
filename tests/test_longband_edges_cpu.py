"""The FFT band engine (csrc/band_fft.h) at the edges of its FFT classes and lengths: a MADE plan (``SliCQPlan`` is a plain dataclass
and the library takes any plan) that puts one band on every edge no scale-built plan reaches.  Owns the plan, the shapes and the
helpers of tests/test_longband_edges_gpu.py, and holds on the CPU that the rule of that module has teeth.

A band of length Lg = 4 m runs a Bluestein transform of length m in a cyclic convolution of N points, N the smallest power of two
>= max(8, 2 m - 1): alias-free only while 2 m - 1 <= N, tightest at m = N / 2 (Lg = 2 N); Lg = 2 N + 4 is the first length of the
next class.  L = 32768, tr = 8192; bands as (Lg, c):

  band 0        324, 0          the DC band on the engine at its smallest length: half the window below bin 0 (mirrored, conjugated)
  band 1, 2     16, 200; 64, 300      short engines beside it
  band 3        320, 600        the boundary: NOT on the FFT engine
  band 4        512, 1000       m 128 fills N 256
  band 5, 6     516 x 2, 1402 / 1800  first length of N 512; F = 2; both signs of (-1)^(c/2)
  band 7, 8, 9  1024 x 3, 2400 / 3002 / 3600    m 256 fills N 512; F = 3
  band 10       1028, 4400      first length of N 1024
  band 11       2048, 5602      fills N 1024
  band 12       2052, 7000      first length of N 2048
  band 13       4096, 9000      fills N 2048
  band 14       4100, 10002     first length of N 4096
  band 15       8192, 12000     fills N 4096
  band 16       8196, 12286     first length of N 8192; its upper edge on bin L / 2
  band 17       16372, 8192     m 4093, a prime, in N 8192
  band 18       16384, 16384    the engine's maximum: fills N 8192; the Nyquist band, half the window mirrored above L / 2

16 bands on the engine in 16 blocks; no band 1 .. 17 has 0 < c < Lg / 2, so no share across DC arises.  The windows are not
smooth: g[q] uniform in [0.5, 1.5] times a random sign (fp32), gd[q] the same in fp64 over Lg, seeded -- every entry of every band
weighs the same, where a Blackman-Harris window multiplies an error at q near Lg / 2 by 1e-5.  They are not dual: nothing here
tests reconstruction; ``ref64`` and the fp32 oracle use them as given.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import ref64
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables

L, TR = 32768, 8192
BANDS = [(324, 0), (16, 200), (64, 300), (320, 600), (512, 1000), (516, 1402), (516, 1800), (1024, 2400), (1024, 3002), (1024, 3600),
         (1028, 4400), (2048, 5602), (2052, 7000), (4096, 9000), (4100, 10002), (8192, 12000), (8196, 12286), (16372, 8192), (16384, 16384)]
BLOCKS = [(0, 1, 324), (1, 1, 16), (2, 1, 64), (3, 1, 320), (4, 1, 512), (5, 2, 516), (7, 3, 1024), (10, 1, 1028), (11, 1, 2048),
          (12, 1, 2052), (13, 1, 4096), (14, 1, 4100), (15, 1, 8192), (16, 1, 8196), (17, 1, 16372), (18, 1, 16384)]
ENGINE_BANDS = [0] + list(range(4, 19))
CLASSES = {324: (81, 256), 512: (128, 256), 516: (129, 512), 1024: (256, 512), 1028: (257, 1024), 2048: (512, 1024), 2052: (513, 2048),
           4096: (1024, 2048), 4100: (1025, 4096), 8192: (2048, 4096), 8196: (2049, 8192), 16372: (4093, 8192), 16384: (4096, 8192)}
FULL = [4, 7, 8, 9, 11, 13, 15, 18]               # 2 m = N
SEED = 20261021
_PLAN = []


def fft_class(Lg):
    """(m, N) by the rule of csrc/band_fft.h: N the smallest power of two >= max(8, 2 m - 1)."""
    m, N = Lg // 4, 8
    while N < 2 * m - 1:
        N *= 2
    return m, N


def edge_plan():
    """(SliCQPlan, oracle.slicqt.Plan) from the one table above."""
    if not _PLAN:
        from xumx_slicq_amd.plan import SliCQPlan
        rng = np.random.default_rng(SEED)
        Lg = np.asarray([b[0] for b in BANDS], dtype=np.int32)
        c = np.asarray([b[1] for b in BANDS], dtype=np.int32)
        g = [(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n in Lg]
        gd = [(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n) / float(n)).astype(np.float64) for n in Lg]
        tw = O.tukey_slice_window(L, TR).numpy()
        pkg = SliCQPlan(scale="edges", fbins=len(BANDS), fmin=0.0, fmax=22050.0, fs=44100.0, L=L, tr=TR, Lg=Lg, c=c, g=np.concatenate(g),
                        gd=np.concatenate(gd), tw=tw, blocks=list(BLOCKS), dc_twins=False, twins=[], long_bands=True)
        orc = O.Plan(fs=44100.0, L=L, tr=TR, nbands=len(BANDS), Lg=Lg.astype(np.int64), c=c.astype(np.int64), g=[a.copy() for a in g],
                     gd=[a.copy() for a in gd], tw=tw.copy(), blocks=list(BLOCKS), twins=[])
        _PLAN.append((pkg, orc))
    return _PLAN[0]


def lengths():
    """n = 2 h + 1 (S = 3) and n = 7 h + 123 (S = 5, ragged tail)."""
    h = L // 4
    return [2 * h + 1, 7 * h + 123]


def audio(n, rows):
    """(rows, n) float32: seeded noise at 0.1."""
    return 0.1 * torch.randn(rows, n, generator=torch.Generator().manual_seed(SEED + n + rows))


def random_blocks(BC, S, seed, lead=None):
    gen = torch.Generator().manual_seed(seed)
    lead = (BC,) if lead is None else tuple(lead)
    return [torch.randn(*lead, F, S, T, 2, generator=gen) for (_, F, T) in BLOCKS]


def one_block_rows(S, seed, real=False):
    """A block list with a leading dimension of nblocks: row k is zero except in block k (seeded normal; ``real``: uniform in
    [0, 1) without the complex pair, a mask) -- the construction of ``one_block_inputs`` of tests/test_ref64_mel_cpu.py, one channel."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k, (_, F, T) in enumerate(BLOCKS):
        p = torch.zeros(len(BLOCKS), F, S, T) if real else torch.zeros(len(BLOCKS), F, S, T, 2)
        p[k] = torch.rand(F, S, T, generator=gen) if real else torch.randn(F, S, T, 2, generator=gen)
        out.append(p)
    return out


def one_band_rows(S, seed):
    """Two rows: the first zero except in band 6 (f = 1 of the F = 2 block), the second zero except in band 9 (f = 2 of the F = 3 block)."""
    gen = torch.Generator().manual_seed(seed)
    out = [torch.zeros(2, F, S, T, 2) for (_, F, T) in BLOCKS]
    out[5][0, 1] = torch.randn(S, 516, 2, generator=gen)
    out[6][1, 2] = torch.randn(S, 1024, 2, generator=gen)
    return out


def band_labels(rows):
    return [f"row {r} band {j} Lg {BANDS[j][0]}" for r in range(rows) for j in range(len(BANDS))]


def block_labels():
    return [f"block {b} F {F} T {T}" for b, (_, F, T) in enumerate(BLOCKS)]


def flat(e):
    return tuple(a.reshape(-1) for a in e)


def block_of(j):
    """(block, f) of band j."""
    for b, (j0, F, _) in enumerate(BLOCKS):
        if j0 <= j < j0 + F:
            return b, j - j0
    raise IndexError(j)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_facts():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.plan import LONG_BAND_MIN, build_plan, dropped_twin_share, long_band_max
    pkg, orc = edge_plan()
    assert _lib.lib.xsq_plan_long_band_min() == LONG_BAND_MIN == 320 and _lib.lib.xsq_plan_long_band_max() == long_band_max() == 16384
    assert (pkg.L, pkg.tr, pkg.nbands, pkg.long_bands, pkg.dc_twins, pkg.twins) == (32768, 8192, 19, True, False, [])
    assert pkg.coefs_per_slice == 67808 and pkg.num_slices(lengths()[0]) == 3 and pkg.num_slices(lengths()[1]) == 5
    # the blocks are the runs of equal length
    runs, j = [], 0
    while j < pkg.nbands:
        k = j
        while k + 1 < pkg.nbands and pkg.Lg[k + 1] == pkg.Lg[j]:
            k += 1
        runs.append((j, k - j + 1, int(pkg.Lg[j])))
        j = k + 1
    assert runs == BLOCKS == pkg.blocks == orc.blocks and len(BLOCKS) == 16 and [F for (_, F, _) in BLOCKS if F > 1] == [2, 3]
    # what the library asks of any plan, and of a long_bands plan
    assert not np.any(pkg.Lg % 4) and not np.any(pkg.c % 2) and int(pkg.Lg.max()) == pkg.L // 2 == long_band_max()
    assert not any(0 < c < n // 2 for (n, c) in BANDS[1:-1]) and float(dropped_twin_share(pkg.L, pkg.Lg, pkg.c, pkg.gd).max()) == 0.0
    # the engine's bands and their classes
    assert [j for j, (n, _) in enumerate(BANDS) if n > LONG_BAND_MIN] == ENGINE_BANDS and len(ENGINE_BANDS) == 16 and BANDS[3][0] == LONG_BAND_MIN
    assert {n: fft_class(n) for (n, _) in BANDS if n > LONG_BAND_MIN} == CLASSES
    assert [j for j in ENGINE_BANDS if 2 * fft_class(BANDS[j][0])[0] == fft_class(BANDS[j][0])[1]] == FULL
    for j in ENGINE_BANDS:                            # every other one is the first length of its class: four less fills the class below
        m, N = fft_class(BANDS[j][0])
        assert 2 * m - 1 <= N and (j in FULL or j in (0, 17) or fft_class(BANDS[j][0] - 4) == (N // 4, N // 2))
    assert all(4093 % p for p in range(2, 64))        # 4093 < 64^2: a prime
    assert sorted({(c // 2) % 2 for (_, c) in BANDS[5:7]}) == [0, 1]
    # the edges in bins: band 0 half below DC, band 16 ends on L / 2, band 18 half above it
    assert BANDS[0][1] - BANDS[0][0] // 2 == -162 and BANDS[16][1] + BANDS[16][0] // 2 == L // 2 and BANDS[18][1] == L // 2
    # the rule of the forward adjoint's fold: every bin outside [0, L / 2] mirrors onto a bin that some band covers (bin 162, the mirror
    # of the DC band's first entry, by band 17 alone)
    cover = np.zeros(L // 2 + 1, dtype=bool)
    for (n, c) in BANDS:
        k = c - n // 2 + np.arange(n)
        cover[k[(k >= 0) & (k <= L // 2)]] = True
    for (n, c) in BANDS:
        k = c - n // 2 + np.arange(n)
        assert cover[-k[k < 0]].all() and cover[L - k[k > L // 2]].all(), (n, c)
    # the slice window is the package's
    mel = build_plan("mel", 32, 115.5)
    assert np.array_equal(O.tukey_slice_window(mel.L, mel.tr).numpy(), mel.tw) and pkg.tw.dtype == np.float32
    # the windows: no entry small, both signs, fp32 / fp64
    assert pkg.g.dtype == np.float32 and pkg.gd.dtype == np.float64 and np.array_equal(np.concatenate(orc.g), pkg.g)
    off = np.concatenate(([0], np.cumsum(pkg.Lg)))
    for j, (n, _) in enumerate(BANDS):
        g, gd = pkg.g[off[j]: off[j + 1]], pkg.gd[off[j]: off[j + 1]] * n
        assert 0.5 <= np.abs(g).min() and np.abs(g).max() <= 1.5 and 0.5 <= np.abs(gd).min() and np.abs(gd).max() <= 1.5
        assert (g < 0).any() and (g > 0).any() and (gd < 0).any() and (gd > 0).any()


# ---- the rule catches one wrong entry ---------------------------------------------------------------------------------------------------
_T = Tables("longband_edges_cpu", {"forward": M_CAP, "inverse": M_CAP})
_CASE = {}


def _forward_case():
    if "fwd" not in _CASE:
        _, plan = edge_plan()
        x = audio(lengths()[0], 1)
        ref = ref64.forward(plan, x)
        cpu = O.forward(plan, x)
        _CASE["fwd"] = (x, ref, cpu, flat(ref64.band_rel_err(cpu, ref, True)))
    return _CASE["fwd"]


def _flagged(got, ref, e_cpu):
    """The labels ``Tables.judge`` reports for ``got``, by the call of tests/test_longband_edges_gpu.py at M = M_CAP."""
    bad, _ = _T.judge("forward", "damaged", flat(ref64.band_rel_err(got, ref, True)), e_cpu, band_labels(1))
    return [m.split(":")[0] for m in bad]


def _swap_radix4_entries(C):
    """(a) band 18: the coefficients k1 + m k2 and k1 + m ((k2 + 2) & 3) swapped for one k1 -- the synthesis' last write, taken for
    the analysis'."""
    b, f = block_of(18)
    m, k1 = 4096, 1234
    band = C[b][:, f]                                             # (a view)
    for k2 in (0, 1):
        lo, hi = k1 + m * k2, k1 + m * (k2 + 2)
        keep = band[:, :, lo].clone()
        band[:, :, lo] = band[:, :, hi]
        band[:, :, hi] = keep
    return 18


def _mirror_without_conjugate(C):
    """(b) band 0 from a spectrum whose mirrored bins (below 0) are read at |bin| and NOT conjugated."""
    _, plan = edge_plan()
    x = _forward_case()[0]
    h, S = plan.h, plan.nslices(x.shape[-1])
    xpad = torch.zeros(1, (2 * S + 2) * h)
    xpad[:, 2 * h: 2 * h + x.shape[-1]] = x
    U = torch.fft.fft(xpad.unfold(-1, L, 2 * h)[:, :S] * torch.from_numpy(plan.tw))
    k = plan.c[0] + O._sq(324)
    t = U[:, :, np.abs(k)] * torch.from_numpy(plan.g[0])          # U[-k] = conj(U[k]) is what the transform reads
    C[0][:, 0] = torch.view_as_real(torch.fft.ifft(t))            # (c = 0: sign +)
    return 0


def _neighbour_of_the_block(C):
    """(c) band 8 (f = 1 of F = 3) holds band 7's values: a kernel that ignores ``f``."""
    b, f = block_of(8)
    C[b][:, f] = C[b][:, f - 1]
    return 8


def _last_output_of_the_convolution(C):
    """(d) band 4 (2 m = N): the sub-transforms' output m - 1 -- the one a convolution of N < 2 m - 1 points aliases first -- zeroed, so
    the four coefficients m - 1 + m k2 lose it."""
    b, f = block_of(4)
    m = 128
    A = torch.fft.fft(torch.view_as_complex(C[b][:, f].contiguous()).reshape(-1, 4, m), dim=1)       # the four A_r w^{r k1} at each k1
    A[:, :, m - 1] = 0
    C[b][:, f] = torch.view_as_real(torch.fft.ifft(A, dim=1).reshape(1, -1, 4 * m))
    return 4


def test_oracle_error_is_flat_over_the_bands():
    """E, the fp32 oracle's error against float64, is neither zero nor noise: every band between one and sixteen fp32 roundings
    (2^-24 = 6e-8) at both shapes, and the largest (band 17: the CPU's own FFT of 4 * 4093 points) within four times the smallest, so
    judging every band against the largest E of the stage gives none of them more than two more bits."""
    _, plan = edge_plan()
    for n, BC in zip(lengths(), (1, 3)):
        x = audio(n, BC)
        ref = ref64.forward(plan, x)
        rms, mx = ref64.band_rel_err(O.forward(plan, x), ref, True)
        print(f"forward n {n}: E rms {rms.min():.3e} .. {rms.max():.3e}, max {mx.max():.3e}")
        assert 6e-8 < rms.min() and rms.max() < 1e-6 and rms.max() < 4 * rms.min()
        X = random_blocks(BC, plan.nslices(n), n)
        r = ref64.inverse(plan, X, n)
        rms, _ = ref64.rel_err(O.inverse(plan, X, n), r, keep=(0,))
        print(f"inverse n {n}: E rms {rms.min():.3e} .. {rms.max():.3e}")
        assert 6e-8 < rms.min() and rms.max() < 1e-6


def test_the_undamaged_output_is_not_flagged():
    _, ref, cpu, e_cpu = _forward_case()
    assert _flagged(cpu, ref, e_cpu) == []


@pytest.mark.parametrize("damage", [_swap_radix4_entries, _mirror_without_conjugate, _neighbour_of_the_block, _last_output_of_the_convolution])
def test_the_rule_catches_one_wrong_entry_of_the_forward_transform(damage):
    """The fp32 oracle's output, damaged the way a subtly wrong kernel would, through the GPU test's own ``judge`` call at M = M_CAP:
    the damaged band is reported, and no other."""
    _, ref, cpu, e_cpu = _forward_case()
    C = [c.clone() for c in cpu]
    j = damage(C)
    assert sum(not torch.equal(a, b) for a, b in zip(C, cpu)) == 1
    assert _flagged(C, ref, e_cpu) == [f"row 0 band {j} Lg {BANDS[j][0]}"]


@pytest.mark.parametrize("j", [0, 6, 12, 18])
def test_the_rule_catches_a_synthesis_window_rolled_by_one(j):
    """The inverse with band j's window rolled by one entry: the band's block is reported among blocks set one at a time, and no other;
    so is every row of random coefficients in all blocks."""
    _, plan = edge_plan()
    wrong = copy.copy(plan)
    wrong.gd = [np.roll(w, 1) if i == j else w for i, w in enumerate(plan.gd)]
    n = lengths()[0]
    P = one_block_rows(3, n)
    ref = ref64.inverse(plan, P, n)
    e_cpu = ref64.rel_err(O.inverse(plan, P, n), ref, keep=(0,))
    bad, _ = _T.judge("inverse", "clean", e_cpu, e_cpu, block_labels())
    assert bad == []
    bad, _ = _T.judge("inverse", "rolled", ref64.rel_err(O.inverse(wrong, P, n), ref, keep=(0,)), e_cpu, block_labels())
    assert [m.split(":")[0] for m in bad] == [block_labels()[block_of(j)[0]]]
    X = random_blocks(2, 3, n + 2)
    ref = ref64.inverse(plan, X, n)
    bad, _ = _T.judge("inverse", "rolled, all blocks", ref64.rel_err(O.inverse(wrong, X, n), ref, keep=(0,)),
                      ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)), ["row 0", "row 1"])
    assert len(bad) == 2
