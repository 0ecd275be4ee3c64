"""oracle/ref64.py on the Mel-32 plan (``fscale = mel, fbins = 32, fmin = 115.5``: the reference's small streaming models) is the
reference's operation, and the inputs of tests/test_ref64_mel_gpu.py are what that module relies on: the plan facts, the Wiener
window geometry of the long clip, an fp32-oracle error E per stage that is neither zero nor noise, and CDAE masks away from the
flat ends of the sigmoid.  No GPU; the constants and input builders of the GPU module live here so both see the same cases.
"""
import contextlib

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64
from oracle import separator as osep
from oracle import slicqt as O
from test_ref64_gpu import _forward_inputs
from test_wiener_iters_cpu import wiener_iters
from test_wiener_options_cpu import EPS, wiener_options
from xumx_slicq_amd.synth import synth_audio

MEL = ("mel", 32, 115.5)
SEED = 77
MEL_BLOCKS = [(9, 16), (2, 20), (1, 24), (2, 28)] + [(1, T) for T in (32, 36, 40, 44, 48, 56, 60, 68, 76, 84, 96, 104, 116, 132, 144,
                                                                        164, 180, 200, 212)]
N_SHORT, N_CHUNK, N_LONG = 1513, 32768, 300000       # S = 3, S = 34 (one streaming chunk), S = 299 (22 blocks of several windows)
WIN = omodel.WIENER_WIN
MASK_LOGIT_SHIFT = 1.5          # tests/test_wiener_options_gpu.py: lowers the last-layer biases so the residual is a source of weight
E_CEIL = 1e-5                   # every fp32-oracle error must lie in (0, E_CEIL): measured 1.5e-7 .. 4e-6


@contextlib.contextmanager
def one_thread():
    """The fp32 oracle's convolutions over rows of 10^4 .. 10^5 positions and one or two channels are tens of times slower on
    several threads than on one (oneDNN splits them badly); the float64 ones are not."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def make_mel_plan():
    return O.make_plan(*MEL)


def make_mel_sd(plan, shift=0.0):
    from xumx_slicq_amd.weights import seeded_state_dict
    sd = seeded_state_dict([(F, T) for (_, F, T) in plan.blocks], seed=SEED)
    if shift:
        sd = {k: (v - shift if k.endswith(".9.bias") else v) for k, v in sd.items()}
    return sd


def audio(n, B=2, loud_row=False):
    x = synth_audio(n, seed=20260101 + n, nb_samples=B)
    if loud_row:
        x[1] *= 40.0
    return x


def one_block_inputs(plan, n):
    """(P, Q): P[k] is zero except in block k (seeded normal), stacked along a leading dimension of nblocks; Q is every block at
    once in the 7-D (4, B, 2, ...) form Unmix returns."""
    S, nb = plan.nslices(n), len(plan.blocks)
    gen = torch.Generator().manual_seed(n)
    P = []
    for k, (_, F, T) in enumerate(plan.blocks):
        p = torch.zeros(nb, 1, 2, F, S, T, 2)
        p[k] = torch.randn(1, 2, F, S, T, 2, generator=gen)
        P.append(p)
    gen = torch.Generator().manual_seed(n + 1)
    Q = [torch.randn(4, 2, 2, F, S, T, 2, generator=gen) for (_, F, T) in plan.blocks]
    return P, Q


def windows(S, T):
    """(number of Wiener windows, frames of the last one) of a block with S slices of T frames."""
    N = S * T
    return -(-N // WIN), N - (-(-N // WIN) - 1) * WIN


def stems_ref(plan, sd, x, causal, wiener, chunk):
    return torch.cat([ref64.separate(plan, sd, x[..., p:p + chunk], causal=causal, wiener=wiener)
                      for p in range(0, x.shape[-1], chunk)], dim=-1)


STEM_MODELS = [("realtime", True, False), ("offline_phasemix", False, False), ("offline_wiener", False, True)]
STEM_CASES = [(500, 32768), (N_SHORT, 32768), (40000, 32768), (N_LONG, 2621440)]          # (n, chunk_size)


def residual_share(pairs):
    """Share of the points of [(X block, masks block)] whose residual magnitude is positive (tests/test_wiener_options_gpu.py)."""
    pos = tot = 0
    for Xb, mb in pairs:
        ax = omodel.abs_of_real_complex(Xb)
        v = mb * ax
        vr = torch.where(ax > EPS, ax, torch.full_like(ax, EPS)) - (((v[0] + v[1]) + v[2]) + v[3])
        pos, tot = pos + int((vr > 0).sum()), tot + vr.numel()
    return pos / tot


def _ok(e, what, max_scale=1.0):
    """Both metrics of every member in (0, E_CEIL); ``max_scale`` widens the ceiling of rel_max alone (see the impulse input)."""
    for a, ceil in zip(e, (E_CEIL, E_CEIL * max_scale)):
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        assert np.all(np.isfinite(a)) and a.min() > 0 and a.max() < ceil, (what, float(a.min()), float(a.max()), ceil)


@pytest.fixture(scope="module")
def plan():
    return make_mel_plan()


@pytest.fixture(scope="module")
def sd(plan):
    return make_mel_sd(plan)


@pytest.fixture(scope="module")
def long_coefs(plan):
    """fp32 oracle coefficients of the long clip, B = 2 with batch row 1 forty times louder."""
    return O.forward(plan, audio(N_LONG, 2, loud_row=True))


# ---- 1. ref64 is the reference's operation ----------------------------------------------------------------------------------------
def test_ref64_forward_and_inverse_match_the_reference_fixture(plan):
    """The bounds tests/test_mel_plan.py holds the fp32 oracle to: 1e-5 on every coefficient, 5e-5 max / 1e-5 RMS on the inverse of
    the perturbed coefficients (the inverse keeps the 2.2e-5 structural difference of the reference's mirror branch, quirk A12)."""
    from test_mel_plan import _pert
    g = load_golden("mel32_32768.npz")
    n = int(g["n"])
    assert n == N_CHUNK
    C = ref64.forward(plan, synth_audio(n, seed=20260101 + n))
    assert len(C) == 23 and C[0].shape[3] == int(g["S"]) == 34 and C[0].dtype == torch.float64
    for i, cb in enumerate(C):
        assert float((cb - torch.from_numpy(g[f"fwd_{i}"])).abs().max()) < 1e-5, i
    y = ref64.inverse(plan, _pert(g, [torch.from_numpy(g[f"fwd_{i}"]) for i in range(23)]), n)
    d = y - torch.from_numpy(g["inv"])
    assert y.dtype == torch.float64 and float(d.abs().max()) < 5e-5 and float(d.pow(2).mean().sqrt()) < 1e-5


# ---- 2. the plan facts the GPU tests rely on ------------------------------------------------------------------------------------------
def test_plan_facts(plan):
    from xumx_slicq_amd.plan import build_plan
    from xumx_slicq_amd.phase import resident_max_window
    assert (plan.L, plan.tr, plan.h, plan.nbands) == (2016, 504, 504, 33)
    assert [(F, T) for (_, F, T) in plan.blocks] == MEL_BLOCKS and len(MEL_BLOCKS) == 23
    assert [tuple(b) for b in build_plan(*MEL).block_shapes()] == MEL_BLOCKS
    assert all(T % 2 == 0 for _, T in MEL_BLOCKS)                       # softmask / residual run two frames per thread
    assert int(plan.Lg.max()) == 212 and int(plan.c[-1]) == plan.L // 2
    assert [plan.nslices(n) for n in (500, 1009, N_SHORT, N_CHUNK, 40000 - N_CHUNK, N_LONG)] == [2, 3, 3, 34, 9, 299]
    S = plan.nslices(N_LONG)
    w = [windows(S, T) for _, T in MEL_BLOCKS]
    assert sum(k > 1 for k, _ in w) >= 20 and any(k > 1 and tail < WIN for k, tail in w)
    assert sum(k > 1 for k, _ in w) == 22 and sum(k > 1 and tail < WIN for k, tail in w) == 22
    assert resident_max_window() >= WIN


# ---- 3. the fp32 oracle's error against ref64, stage by stage ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_SHORT, N_CHUNK, N_LONG])
def test_oracle_error_of_the_forward_transform(plan, n):
    """rel_rms of every (row, channel, band) is below E_CEIL on every input.  rel_max = max|d| / rms(ref) is so on 'synth' and
    'scaled'; on 'impulse' its ceiling is E_CEIL * sqrt(S / 2): a sample lies in two of the S slices (L = 4h, hop 2h), so the
    reference of a row is zero in the other S - 2 and its RMS over all S is sqrt(2 / S) of the RMS where it is not, while the
    largest error is unchanged."""
    S = plan.nslices(n)
    for name, (x, per_row) in _forward_inputs(plan, n).items():
        _ok(ref64.band_rel_err(O.forward(plan, x), ref64.forward(plan, x), per_row), f"forward n={n} {name}",
            max_scale=max(1.0, (S / 2) ** 0.5) if name == "impulse" else 1.0)


@pytest.mark.parametrize("n", [N_SHORT, N_CHUNK])
def test_oracle_error_of_the_inverse_transform(plan, n):
    for tag, X in zip(("one block", "all blocks"), one_block_inputs(plan, n)):
        _ok(ref64.rel_err(O.inverse(plan, X, n), ref64.inverse(plan, X, n), keep=(0,)), f"inverse n={n} {tag}")


@pytest.mark.parametrize("n,B", [(N_SHORT, 2), (N_CHUNK, 2), (N_LONG, 1)])
def test_oracle_error_of_the_cdae_and_mask_spread(plan, sd, n, B):
    """At least half of the float64 mask values of every block lie in (0.02, 0.98): a saturated sigmoid would hide layer-4 errors."""
    X = O.forward(plan, audio(n, B))
    for causal in (False, True):
        ref = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(X)]
        with one_thread():
            got = [omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(X)]
        _ok(tuple(zip(*(ref64.rel_err(a, r) for a, r in zip(got, ref)))), f"cdae n={n} causal={causal}")
        share = [float(((r > 0.02) & (r < 0.98)).double().mean()) for r in ref]
        print(f"n={n} causal={causal}: share of masks in (0.02, 0.98) per block: min {min(share):.3f}")
        assert min(share) >= 0.5, (n, causal, share)


def test_oracle_error_of_the_wiener_filter_and_residual_share(plan, sd, long_coefs):
    """One iteration, two iterations, and softmask + residual on the masks of the model with lowered last-layer biases, whose
    residual must be positive on a share of the points that is neither negligible nor all of them."""
    sds = make_mel_sd(plan, MASK_LOGIT_SHIFT)
    c1, c2, co, pairs = [], [], [], []
    with one_thread():
        for b, Xb in enumerate(long_coefs):
            mag = omodel.abs_of_real_complex(Xb)
            Ymag = omodel.cdae_masks(sd, b, mag, False) * mag
            c1.append(ref64.rel_err(omodel.blockwise_wiener(Xb, Ymag), ref64.blockwise_wiener(Xb, Ymag)))
            c2.append(ref64.rel_err(wiener_iters(Xb, Ymag, 2, dtype=torch.complex64), wiener_iters(Xb, Ymag, 2)))
            ms = omodel.cdae_masks(sds, b, mag, False)
            pairs.append((Xb, ms))
            co.append(ref64.rel_err(wiener_options(Xb, ms * mag, 1, True, True, dtype=torch.complex64), wiener_options(Xb, ms * mag, 1, True, True)))
    # rel_rms is below E_CEIL in every block of every form (1.1e-7 .. 4.9e-7).  rel_max is so for one iteration and for the options
    # (3.3e-6 .. 9.4e-6); after two iterations it is so in 22 blocks (4.4e-6 .. 8.8e-6) and 2.8e-5 at block 0 (the second pass
    # works on the first one's rounded output; a peak over 0.7 million coefficients): that form's rel_max ceiling is 10 * E_CEIL, and at
    # most one block may be above E_CEIL.
    for tag, c, scale in (("niter 1", c1, 1.0), ("niter 2", c2, 10.0), ("softmask residual", co, 1.0)):
        _ok(tuple(zip(*c)), f"wiener {tag}", max_scale=scale)
    assert sum(float(m) >= E_CEIL for _, m in c2) <= 1
    share = residual_share(pairs)
    print(f"share of points with a positive residual: {share:.3f}")
    assert 0.1 <= share <= 0.9, share


@pytest.mark.parametrize("n,chunk", STEM_CASES)
def test_oracle_error_of_the_stems(plan, sd, n, chunk):
    x = audio(n, 1)
    for name, causal, wiener in STEM_MODELS:
        ref = stems_ref(plan, sd, x, causal, wiener, chunk)
        with one_thread():
            orc = osep.separate(plan, sd, x, causal=causal, wiener=wiener, chunk_size=chunk)
        assert ref.shape == orc.shape == (4, 1, 2, n)
        _ok(ref64.rel_err(orc, ref, keep=(0,)), f"stems {name} n={n}")
