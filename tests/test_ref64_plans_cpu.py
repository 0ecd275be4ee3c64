"""Plans other than the two shipped ones (Bark-262, Mel-32), held to the reference and to float64.  No GPU; this module owns the
plans, the cases and the input builders that tests/test_ref64_plans_gpu.py runs.

Three plans, chosen for the kernel classes they reach (fs 44100, fmax 22050, what ``NSGTBase(scale, fbins, fmin)`` builds):

  T  bark, 28, 32.9     L 1872   first block (10, 16): F = 10 (three taps, F2 = 6); bands 1 and 2 reach across DC
  K  bark, 56, 32.9     L 3808   first block (20, 16): F = 20 (five taps, F1 = 16, F2 = 12); bands 1 and 2 reach across DC
  W  bark, 400, 300.0   L 27496  band 0 has Lg = 376 > 320 and is a block of its own; five-tap blocks (115, 16), (22, 20); three-tap
                                 blocks with T up to 44, so layer 4 leaves F(2, 2) for the whole model; no band reaches across DC

Where a band j >= 1 reaches across DC (0 < c_j < Lg_j / 2) the reference's inverse keeps a second, mirrored synthesis of it
(nsgt/nsigtf.py:57-99, quirk A12).  oracle/slicqt.py and oracle/ref64.py restate it (``plan.twins``); the kernels do not compute it,
so the library REFUSES the plans on which it is not negligible (share >= TWIN_SHARE_MAX: T, K and ``bark, 96, 32.9``) and accepts
the others (Mel-32 at 0.0084, where it drops the term by contract).  T and K are therefore CPU cases, and on the GPU they appear as
refused; the GPU parity of this round runs on W and on M = ``mel, 64, 115.5`` (L 4096, first blocks (1, 20), (16, 16); no band
reaches across DC).  Measured distances of the inverse from the reference fixture, max-abs on the S = 3 clip (forward's output /
block 0 alone / seeded normal coefficients): T without the mirrored term 5.2e-3 / 5.2e-3 / 3.7e-3, with it 1.8e-7 / 1.5e-7 / 9.1e-7;
K 1.1e-3 / 1.1e-3 without, 1.8e-7 / 1.7e-7 with.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64
from oracle import separator as osep
from oracle import slicqt as O
from test_ref64_gpu import _forward_inputs
from test_ref64_mel_cpu import E_CEIL, _ok, one_block_inputs, one_thread, stems_ref, windows
from xumx_slicq_amd.synth import synth_audio

PLANS = {"T": ("bark", 28, 32.9), "K": ("bark", 56, 32.9), "W": ("bark", 400, 300.0), "M": ("mel", 64, 115.5)}
ISSUE_PLANS = ("T", "K", "W")               # the class-coverage argument is over these three
GPU_PLANS = ("W", "M")                      # accepted by the library
REFUSED = {"T": 1, "K": 1}                  # name -> the band the refusal names
SEED = 77
RANDOM_SEED = 2803                          # oracle/make_golden_plans.py
STEM_MODELS = [("realtime", True, False), ("offline_phasemix", False, False), ("offline_wiener", False, True)]
LONG_E_BLOCKS = list(range(9)) + [27, 36, 54, 61]      # W at S = 66 / 65: E over blocks 0..8 plus four one-tap blocks
TRAIN_MODELS = {"offline+wiener": (False, True), "causal+mixphase": (True, False)}
TRAIN_B = {"W": 1, "M": 2}
RISK, LOOSE_SHARE = 3e-6, 0.02              # tests/test_ref64_train_gpu.py
TENSORS_PER_GROUP = 11                      # conv, BatchNorm and bias tensors of one (block, target); 2 whitening tensors per block

FACTS = {   # name: (L, h, nbands, band 0 Lg, largest Lg, bands reaching across DC, l4f_fits, block shapes)
    "T": (1872, 468, 29, 16, 272, [1, 2], True,
          [(10, 16), (2, 20)] + [(1, T) for T in (24, 28, 32, 40, 44, 52, 60, 72, 84, 100, 116, 136, 156, 184, 216, 252, 272)]),
    "K": (3808, 952, 57, 16, 284, [1, 2], True,
          [(20, 16), (2, 20), (3, 24), (2, 28), (1, 32), (2, 36)] + [(1, T) for T in (40, 44, 48, 52, 56, 60, 64, 68, 72, 80, 84, 92, 100, 108, 116, 128,
                                                                                      136, 148, 160, 172, 184, 200, 216, 232, 252, 272, 284)]),
    "W": (27496, 6874, 401, 376, 376, [], False,
          [(1, 376), (115, 16), (22, 20), (19, 24), (15, 28), (13, 32), (12, 36), (11, 40), (10, 44), (8, 48), (8, 52), (8, 56), (7, 60), (7, 64), (6, 68),
           (6, 72), (5, 76), (5, 80), (5, 84), (5, 88), (5, 92), (4, 96), (4, 100), (4, 104), (4, 108), (4, 112), (4, 116), (3, 120), (3, 124), (4, 128),
           (3, 132), (3, 136), (3, 140), (3, 144), (3, 148), (2, 152), (3, 156), (3, 160), (2, 164), (3, 168), (2, 172), (3, 176), (2, 180), (2, 184),
           (2, 188), (3, 192), (2, 196), (2, 200), (2, 204), (2, 208), (2, 212), (2, 216), (2, 220), (2, 224), (1, 228), (2, 232), (2, 236), (2, 240),
           (1, 244), (2, 248), (2, 252), (1, 256), (3, 260)]),
    "M": (4096, 1024, 65, 20, 216, [], True,
          [(1, 20), (16, 16), (4, 20), (3, 24), (2, 28), (3, 32), (2, 36), (2, 40), (2, 44), (1, 48), (2, 52), (1, 56), (1, 60), (1, 64), (2, 68)]
          + [(1, T) for T in (72, 76, 80, 88, 92, 96, 100, 108, 112, 120, 124, 132, 140, 148, 156, 164, 172, 180, 192, 200, 212, 216)]),
}
# the weight of the mirrored synthesis relative to the band's own (xsq_slicqt_dropped_twin_share), largest band of the plan
SHARES = {("bark", 262, 32.9): 0.0, ("mel", 32, 115.5): 0.0084, ("bark", 28, 32.9): 0.317, ("bark", 56, 32.9): 0.317, ("bark", 96, 32.9): 0.109,
          ("bark", 400, 300.0): 0.0, ("mel", 64, 115.5): 0.0}


def kf_of(F):
    """xumx_slicq_amd/csrc/cdae.hip (kf_of) and train.hip (kf_of_t): taps along the frequency axis."""
    return 1 if F < 10 else (3 if F < 20 else 5)


def l4f_fits(shapes):
    """cdae_launch_layer (cdae.hip): layer 4 runs as F(2, 2) only if no block with several frequency taps is wider than 32."""
    return all(kf_of(F) == 1 or T <= 32 for F, T in shapes)


@functools.lru_cache(maxsize=None)
def make_plan(name):
    return O.make_plan(*PLANS[name])


@functools.lru_cache(maxsize=None)
def make_sd(name):
    from xumx_slicq_amd.weights import seeded_state_dict
    return seeded_state_dict([(F, T) for (_, F, T) in make_plan(name).blocks], seed=SEED)


def n_for(plan, S):
    """n = 4h - 77 for S = 3, (2S - 2)h - 977 for a larger S."""
    n = 4 * plan.h - 77 if S == 3 else (2 * S - 2) * plan.h - 977
    assert plan.nslices(n) == S
    return n


def audio(n, B=2):
    return synth_audio(n, seed=20260101 + n, nb_samples=B)


def train_inputs(name, plan, base):
    """(x, y_t) of one training step: the sum of four seeded sources at S = 3 (tests/test_ref64_train_gpu.py: _inputs)."""
    n, B = n_for(plan, 3), TRAIN_B.get(name, 2)
    y_t = torch.stack([0.5 * synth_audio(n, seed=base + j, nb_samples=B) for j in range(4)])
    return y_t.sum(0), y_t


def near_kink_tensors(plan, sd, X, Yt, causal, wiener):
    """(tensors in near-kink groups, all tensors, groups): a (block, target) group whose smallest float64 |BatchNorm output| is below
    RISK makes its 11 tensors and the two whitening tensors of its block candidates for the loose bound of the training judge."""
    _, _, grads, minima, _ = ref64.training_gradients(plan, sd, X, Yt, causal, wiener)
    groups = {k.rsplit(".", 1)[0] for k, v in minima.items() if v < RISK}
    blocks = {g.split(".cdaes.")[0] for g in groups}
    return TENSORS_PER_GROUP * len(groups) + 2 * len(blocks), len(grads), sorted(groups)


def train_seed_base(name):
    """The first of 600, 610, 620, ... at which at most LOOSE_SHARE of the tensors of BOTH models lie in near-kink groups.  W: at 600
    the offline model has 5 groups in 4 blocks, 63 of 2898 tensors (the cap is 57), the causal one 52; at 610 they have 26 and 13."""
    return {"W": 610, "M": 600, "T": 600, "K": 600}[name]


def random_coefs(plan, S, seed=RANDOM_SEED):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(1, 2, F, S, T, 2, generator=gen) for (_, F, T) in plan.blocks]


def fixture_coefs(name, g):
    return [torch.from_numpy(g[f"fwd_{i}"]) for i in range(len(FACTS[name][7])) if f"fwd_{i}" in g]


# ---- 1. plan facts and class coverage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PLANS))
def test_plan_facts(name):
    L, h, nbands, lg0, lgmax, crossing, fits, shapes = FACTS[name]
    p = make_plan(name)
    g = load_golden(f"plans3_{name}.npz")
    assert (p.L, p.h, p.tr, p.nbands) == (L, h, h, nbands) == (int(g["L"]), int(g["L"]) // 4, int(g["tr"]), int(g["nbands"]))
    assert [(F, T) for (_, F, T) in p.blocks] == shapes == [tuple(b) for b in g["blocks"].tolist()]
    assert np.array_equal(p.Lg, g["Lg"]) and np.array_equal(p.c % L, g["c"])
    assert (int(p.Lg[0]), int(p.Lg.max())) == (lg0, lgmax)
    assert [j for j in range(1, nbands - 1) if 0 < p.c[j] < p.Lg[j] // 2] == crossing == [t[0] for t in p.twins]
    assert l4f_fits(shapes) == fits
    assert int(g["n"]) == n_for(p, 3) == 4 * h - 77 and int(g["S"]) == 3
    if name == "W":
        assert (n_for(p, 66), n_for(p, 65)) == (892643, 878895)
    assert all(T % 4 == 0 and F - 2 * (kf_of(F) - 1) >= 1 for F, T in shapes)           # what xsq_model_create requires


def test_the_three_plans_cover_the_classes():
    """Fails if a plan is dropped or swapped for one that loses a class."""
    assert set(ISSUE_PLANS) <= set(PLANS) and [PLANS[k] for k in ISSUE_PLANS] == [("bark", 28, 32.9), ("bark", 56, 32.9), ("bark", 400, 300.0)]
    shapes = [s for k in ISSUE_PLANS for s in FACTS[k][7]]
    Fs = {F for F, _ in shapes}
    assert {10, 19, 20} <= Fs
    assert FACTS["T"][7][0] == (10, 16) and FACTS["K"][7][0] == (20, 16)
    assert any(kf_of(F) == 5 and F > 86 for F, _ in shapes) and any(kf_of(F) == 5 and T > 16 for F, T in shapes)
    assert any(kf_of(F) == 3 and T > 32 for F, T in shapes)
    assert max(FACTS[k][4] for k in ISSUE_PLANS) > 320 and FACTS["W"][3] == 376 and FACTS["W"][7][0] == (1, 376)
    assert max(FACTS[k][0] for k in ISSUE_PLANS) > 18060
    assert not FACTS["W"][6] and FACTS["T"][6] and FACTS["K"][6]                          # only W turns layer 4's F(2, 2) off
    assert FACTS["T"][5] == FACTS["K"][5] == [1, 2] and FACTS["W"][5] == FACTS["M"][5] == []
    # what the GPU plans keep of that: everything but F = 20 and the bands across DC (the library refuses T and K)
    gshapes = [s for k in GPU_PLANS for s in FACTS[k][7]]
    assert {10, 19} <= {F for F, _ in gshapes} and any(kf_of(F) == 3 and T > 32 for F, T in gshapes) and (16, 16) in gshapes


# ---- 2. the library refuses what it would decode differently ----------------------------------------------------------------------------
def test_dropped_twin_share_and_refusal():
    """The share from gd alone (numpy and the library's host function) equals the one from the mirrored band's own dual window;
    build_plan and xsq_plan_create refuse T, K and bark 96 naming band 1, and accept Bark-262, Mel-32, W and M."""
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd import plan as P
    assert P.TWIN_SHARE_MAX == O.TWIN_SHARE_MAX == 0.03
    for cfg, want in SHARES.items():
        op = O.make_plan(*cfg)
        gd = np.concatenate(op.gd)
        Lg, c = op.Lg.astype(np.int32), op.c.astype(np.int32)
        share = P.dropped_twin_share(op.L, Lg, c, gd)
        out, worst = np.empty(len(Lg)), np.zeros(1, dtype=np.int32)
        _lib.check(_lib.lib.xsq_slicqt_dropped_twin_share(op.L, len(Lg), Lg.ctypes.data, c.ctypes.data, gd.ctypes.data, out.ctypes.data,
                                                          worst.ctypes.data), "xsq_slicqt_dropped_twin_share")
        np.testing.assert_allclose(out, share, rtol=1e-12, atol=0)
        np.testing.assert_allclose(share, op.twin_share(), rtol=1e-5, atol=0)             # the frame diagonal is even to fp32 rounding of g
        assert abs(float(share.max()) - want) <= 0.01 * want + 1e-12, (cfg, float(share.max()))
        print(f"{cfg}: share per band across DC {[(j, round(float(s), 5)) for j, s in enumerate(share) if s > 0]}")
        refused = want >= P.TWIN_SHARE_MAX
        assert bool(op.live_twins()) == refused
        g32, tw = np.concatenate(op.g).astype(np.float32), op.tw.astype(np.float32)
        handle = ctypes.c_void_p()
        if refused:
            assert int(worst[0]) == 1
            with pytest.raises(ValueError, match=r"band 1 \(centre bin \d+, Lg 16\) reaches across DC"):
                P.build_plan(*cfg)
            rc = _lib.lib.xsq_plan_create(ctypes.byref(handle), op.L, op.tr, len(Lg), Lg.ctypes.data, c.ctypes.data, g32.ctypes.data, gd.ctypes.data,
                                          tw.ctypes.data)
            assert rc < 0 and not handle.value and "band 1 " in _lib.last_error() and "refused" in _lib.last_error(), _lib.last_error()
        else:
            assert [tuple(b) for b in P.build_plan(*cfg).block_shapes()] == [(F, T) for (_, F, T) in op.blocks]
    assert SHARES[("mel", 32, 115.5)] < P.TWIN_SHARE_MAX < SHARES[("bark", 96, 32.9)]


# ---- 3. reference first -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PLANS))
def test_ref64_and_the_oracle_match_the_reference_fixture(name):
    """The bounds of tests/test_mel_plan.py and tests/test_ref64_mel_cpu.py: 1e-5 on every forward coefficient, 5e-5 max / 1e-5 RMS
    on the decoded waveform -- of the forward's own output, of block 0 alone, and (T) of seeded normal coefficients."""
    p, g = make_plan(name), load_golden(f"plans3_{name}.npz")
    n = int(g["n"])
    x = synth_audio(n, seed=20260101 + n)
    C = fixture_coefs(name, g)
    nb = len(p.blocks)
    assert len(C) == (9 if name == "W" else nb)
    for fwd in (ref64.forward, O.forward):
        got = fwd(p, x)
        for i, cb in enumerate(got):
            if i < len(C):
                assert float((cb - C[i]).abs().max()) < 1e-5, (name, i)
            s = cb.double().flatten()
            np.testing.assert_allclose([float(s.sum()), float((s * s).sum()), float(s.abs().max())], g["fwd_sums"][i], rtol=2e-4, atol=1e-4)
    full = C if len(C) == nb else [c.float() for c in ref64.forward(p, x)]                  # (W: the fixture keeps blocks 0..8 whole)
    alone = [c if i == 0 else torch.zeros_like(c) for i, c in enumerate(full)]
    cases = [("inv", full), ("inv_block0", alone)]
    if name == "T":
        R = random_coefs(p, 3)
        s = [r.double().flatten() for r in R]
        np.testing.assert_allclose([[float(a.sum()), float((a * a).sum()), float(a.abs().max())] for a in s], g["random_sums"], rtol=1e-12)
        cases.append(("inv_random", R))
    for key, X in cases:
        want = torch.from_numpy(g[key])
        for inv in (ref64.inverse, O.inverse):
            d = inv(p, X, n).double() - want
            mx, rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
            print(f"{name} {key} {inv.__module__}: max {mx:.2e} rms {rms:.2e}")
            assert mx < 5e-5 and rms < 1e-5, (name, key, inv.__module__, mx, rms)
        if name in REFUSED:                      # without the mirrored synthesis: the figures of the module docstring
            d = ref64.inverse(p, X, n, twins=False) - want
            assert float(d.abs().max()) > 1e-3, (name, key, float(d.abs().max()))


def test_the_mirrored_synthesis_is_the_references_on_mel32_too():
    """Mel-32 is accepted (share 0.0084) and decoded WITHOUT the term by the library and by the oracle's default; with it the oracle
    comes from 2.2e-5 to fp32 rounding of the reference's decode of the perturbed coefficients (tests/golden/mel32_32768.npz)."""
    from test_mel_plan import _pert
    p, g = O.make_plan("mel", 32, 115.5), load_golden("mel32_32768.npz")
    n = int(g["n"])
    X = _pert(g, [torch.from_numpy(g[f"fwd_{i}"]) for i in range(23)])
    want = torch.from_numpy(g["inv"])
    assert not p.live_twins() and [t[0] for t in p.twins] == [1]
    assert torch.equal(ref64.inverse(p, X, n), ref64.inverse(p, X, n, twins=False))
    without = float((ref64.inverse(p, X, n) - want).abs().max())
    with_ = float((ref64.inverse(p, X, n, twins=True) - want).abs().max())
    print(f"Mel-32 perturbed coefficients: without the term {without:.2e}, with it {with_:.2e}")
    assert 1e-5 < without < 5e-5 and with_ < 2e-6


def test_plans_without_a_band_across_dc_do_not_move():
    """Bark-262, W and M have no twin: the keyword changes nothing, bit for bit."""
    for cfg in (("bark", 262, 32.9), PLANS["W"], PLANS["M"]):
        p = O.make_plan(*cfg)
        assert p.twins == []
        X = random_coefs(p, 3, seed=5)
        for inv in (ref64.inverse, O.inverse):
            assert torch.equal(inv(p, X, 4 * p.h - 77), inv(p, X, 4 * p.h - 77, twins=True))


# ---- 4. the fp32 oracle's error E of every stage the GPU module judges is neither zero nor noise -------------------------------------
@pytest.mark.parametrize("name", list(PLANS))
def test_oracle_error_of_the_transforms(name):
    p = make_plan(name)
    n = n_for(p, 3)
    for inp, (x, per_row) in _forward_inputs(p, n).items():
        _ok(ref64.band_rel_err(O.forward(p, x), ref64.forward(p, x), per_row), f"{name} forward {inp}", max_scale=(3 / 2) ** 0.5 if inp == "impulse" else 1.0)
    for tag, X in zip(("one block", "all blocks"), one_block_inputs(p, n)):
        _ok(ref64.rel_err(O.inverse(p, X, n), ref64.inverse(p, X, n), keep=(0,)), f"{name} inverse {tag}")


@pytest.mark.parametrize("name", list(PLANS))
def test_oracle_error_of_the_cdae_wiener_and_stems_at_three_slices(name):
    p, sd = make_plan(name), make_sd(name)
    n = n_for(p, 3)
    X = O.forward(p, audio(n, 2))
    for causal in (False, True):
        ref = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(X)]
        with one_thread():
            got = [omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(X)]
        _ok(tuple(zip(*(ref64.rel_err(a, r) for a, r in zip(got, ref)))), f"{name} cdae causal={causal}")
        if not causal:
            e = []
            for Xb, m in zip(X, got):
                Ymag = m * omodel.abs_of_real_complex(Xb)
                e.append(ref64.rel_err(omodel.blockwise_wiener(Xb, Ymag), ref64.blockwise_wiener(Xb, Ymag)))
            _ok(tuple(zip(*e)), f"{name} wiener")
    x = audio(n, 1)
    for model, causal, wiener in STEM_MODELS:
        with one_thread():
            orc = osep.separate(p, sd, x, causal=causal, wiener=wiener, chunk_size=2621440)
        _ok(ref64.rel_err(orc, stems_ref(p, sd, x, causal, wiener, 2621440), keep=(0,)), f"{name} stems {model}")


def test_oracle_error_and_mask_spread_of_the_long_case_of_w():
    """W at S = 66 (offline) and S = 65 (causal), B = 2: rows of 131 / 128 positions.  At least 25 % of the float64 mask values of EVERY
    block lie in (0.02, 0.98) (the floor of tests/test_stress_weights_cpu.py; measured worst block 0.43); E over LONG_E_BLOCKS; and
    the Wiener windows of S = 66: one or two windows per block, the T = 376 block among them."""
    p, sd = make_plan("W"), make_sd("W")
    shapes = FACTS["W"][7]
    assert all(kf_of(shapes[b][0]) > 1 for b in range(1, 9)) and all(kf_of(shapes[b][0]) == 1 for b in LONG_E_BLOCKS[9:])
    w = [windows(66, T) for _, T in shapes]
    assert w[0][0] == 5 and w[1] == (1, 66 * 16) and sum(k > 1 and tail < 5000 for k, tail in w) >= 40
    for causal, S in ((False, 66), (True, 65)):
        X = O.forward(p, audio(n_for(p, S), 2))
        ref = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(X)]
        share = [float(((r > 0.02) & (r < 0.98)).double().mean()) for r in ref]
        print(f"W S={S} causal={causal}: share of masks in (0.02, 0.98): worst block {min(share):.3f}")
        assert min(share) >= 0.25, (S, share)
        with one_thread():
            got = [omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(X[b]), causal) for b in LONG_E_BLOCKS]
        _ok(tuple(zip(*(ref64.rel_err(a, ref[b]) for a, b in zip(got, LONG_E_BLOCKS)))), f"W cdae S={S}")


# ---- 5. training batches: the near-kink groups cannot hide a failure -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["T", "K", "W", "M"])
def test_near_kink_groups_stay_under_the_loose_share(name):
    p, sd = make_plan(name), make_sd(name)
    base = train_seed_base(name)
    x, y_t = train_inputs(name, p, base)
    X, Yt = O.forward(p, x), O.forward(p, y_t)
    for model, (causal, wiener) in TRAIN_MODELS.items():
        risky, total, groups = near_kink_tensors(p, sd, X, Yt, causal, wiener)
        print(f"{name} seeds {base}.. {model}: {len(groups)} near-kink groups {groups[:4]}, {risky} of {total} tensors")
        assert total == len(p.blocks) * (4 * TENSORS_PER_GROUP + 2)
        assert risky <= LOOSE_SHARE * total, (name, model, base, groups)


# ---- 6. the adjoint windows on these plans (the closed forms the GPU adjoints are judged by) -------------------------------------------
@pytest.mark.parametrize("name", ["W", "M", "T"])
def test_adjoint_windows_equal_float64_autograd_through_ref64(name):
    """tests/test_sdr_cpu.py and tests/test_autograd_cpu.py on these plans: the window a' of the inverse's adjoint and the window of
    the forward's adjoint (host arithmetic of the library) against float64 autograd through ``ref64.inverse`` / ``ref64.forward``,
    1e-12 allowed.  On T the forward's adjoint holds too, and the inverse's does NOT: autograd goes through the reference's operation,
    mirrored synthesis included, which a' has no term for -- the adjoint of a refused plan is as undefined as its inverse."""
    from test_autograd_cpu import autograd_forward_adjoint, forward_adjoint_closed_form, random_cotangents
    from test_sdr_cpu import adjoint_closed_form, adjoint_window, autograd_adjoint
    p = make_plan(name)
    n = n_for(p, 3)
    G = random_cotangents(p, 2, 3, seed=7 + n % 101)
    ref = autograd_forward_adjoint(p, G, n)
    worst_f = float((forward_adjoint_closed_form(p, G, n) - ref).abs().max() / ref.abs().max())
    gy, ref, S = autograd_adjoint(p, 2, n, seed=5)
    got = adjoint_closed_form(p, adjoint_window(p), gy, S)
    worst_i = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, ref))
    print(f"{name}: forward adjoint {worst_f:.2e}, inverse adjoint {worst_i:.2e} (relative to the largest gradient)")
    assert worst_f <= 1e-12
    if name in REFUSED:
        assert worst_i > 1e-3, worst_i
    else:
        assert worst_i <= 1e-12
