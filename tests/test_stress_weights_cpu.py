"""Conditions on the trained-like weights of oracle/stress.py (reference side only): the floors that make the float64 comparison of
tests/test_ref64_stress_gpu.py meaningful.  The rule has to stress what a trained checkpoint stresses -- dead channels whose
running variance is below eps, signed and zero gammas, masks pinned at 0 and 1 -- and must still leave most of every block away
from saturation, where an error of the kernels shows in the mask.  The assertions are floors, not measured values; if a change of
the draw lands outside one, the seed changes, not the floor.  Measured with seed 4321 (offline / causal): docstrings below.
"""
import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import ref64
from oracle import stress
from xumx_slicq_amd.synth import synth_audio

N, B = 9031, 2


@pytest.fixture(scope="module")
def raw_sd(oracle_plan):
    return stress.stress_state_dict([(F, T) for (_, F, T) in oracle_plan.blocks])


@pytest.fixture(scope="module")
def calibrated_sds(oracle_plan, raw_sd):
    clip = stress.calibration_clip()
    return {causal: stress.calibrated(raw_sd, oracle_plan, causal, clip) for causal in (False, True)}


@pytest.fixture(scope="module")
def coefficients(oracle_plan):
    x = synth_audio(N, seed=20260101 + N, nb_samples=B)
    return ref64.forward(oracle_plan, x)


def _masks(sd, X, causal):
    """(float64 masks, fp32 oracle masks) of every block; the fp32 oracle starts from the coefficients rounded to fp32."""
    X32 = [x.float() for x in X]
    m64 = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(x), causal) for b, x in enumerate(X32)]
    with torch.no_grad():
        m32 = [omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(x), causal) for b, x in enumerate(X32)]
    return m64, m32


@pytest.fixture(scope="module")
def masks(calibrated_sds, coefficients):
    return {causal: _masks(sd, coefficients, causal) for causal, sd in calibrated_sds.items()}


def test_keys_shapes_and_order_are_those_of_the_seeded_rule(raw_sd, calibrated_sds, seeded_sd):
    for sd in (raw_sd, *calibrated_sds.values()):
        assert list(sd) == list(seeded_sd)
        assert all(sd[k].shape == v.shape and sd[k].dtype == v.dtype for k, v in seeded_sd.items())
        assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())


def test_stress_dicts_load_into_the_reference_layout_model(calibrated_sds, oracle_plan):
    from xumx_slicq_amd.separator import build_models
    m, _, _ = build_models(device="cpu")
    for sd in (*calibrated_sds.values(), stress.stress_state_dict(m.table.shapes, dead=False)):
        m.load_state_dict(sd, strict=True)
        got = m.state_dict()
        assert all(torch.equal(got[k], v) for k, v in sd.items())


@pytest.mark.parametrize("causal", [False, True])
def test_every_block_keeps_a_quarter_of_its_mask_values_away_from_saturation(masks, causal):
    """Measured: worst block 52.7 % (offline, block 33) / 48.3 % (causal, block 45), median block 66 % / 63 %."""
    mid = np.array([float(((m > 0.02) & (m < 0.98)).double().mean()) for m in masks[causal][0]])
    print(f"mid-range share: worst block {mid.min():.3f} (block {int(mid.argmin())}), median {np.median(mid):.3f}")
    assert mid.min() >= 0.25, (int(mid.argmin()), mid.min())


@pytest.mark.parametrize("causal", [False, True])
def test_the_median_block_has_masks_pinned_at_both_ends(masks, causal):
    """Measured: median block 2.0 % / 1.7 % of its values below 1e-4 / above 1 - 1e-4 (offline), 2.7 % / 2.2 % (causal); up to 9 %."""
    lo = np.array([float((m < 1e-4).double().mean()) for m in masks[causal][0]])
    hi = np.array([float((m > 1 - 1e-4).double().mean()) for m in masks[causal][0]])
    print(f"share < 1e-4: median {np.median(lo):.4f} max {lo.max():.4f};  share > 1 - 1e-4: median {np.median(hi):.4f} max {hi.max():.4f}")
    assert np.median(lo) >= 0.005 and np.median(hi) >= 0.005, (np.median(lo), np.median(hi))


@pytest.mark.parametrize("causal", [False, True])
def test_running_variances_below_eps_and_signed_gammas(calibrated_sds, causal):
    """Measured: 23 % of the running variances below eps (range 0 .. 8.7e4, median 1.8e-3), 33 % of the gammas negative, 5.0 % zero."""
    sd = calibrated_sds[causal]
    rv = torch.cat([v for k, v in sd.items() if k.endswith("running_var")])
    gamma = torch.cat([v for k, v in sd.items() if k.endswith((".1.weight", ".4.weight", ".7.weight"))])
    assert gamma.numel() == rv.numel() == 70 * 4 * 151
    below, neg, zero = (float(t.double().mean()) for t in (rv < omodel.BN_EPS, gamma < 0, gamma == 0))
    print(f"running_var: {below:.3f} below eps, range {float(rv.min()):.3e} .. {float(rv.max()):.3e}, median {float(rv.median()):.3e}; "
          f"gamma: {neg:.3f} negative, {zero:.3f} zero")
    assert below >= 0.10 and neg >= 0.20 and zero >= 0.02, (below, neg, zero)
    assert float(rv.min()) >= 0.0


def test_a_dead_layer_3_channel_has_zero_running_statistics(raw_sd, calibrated_sds):
    """What the exact tests of the GPU file start from: a zero-gain output channel of `6.weight` has running_mean = running_var = 0."""
    b, t, c = stress.first_dead_channel(raw_sd)
    for sd in calibrated_sds.values():
        p = f"sliced_umx.{b}.cdaes.{t}.7."
        assert float(sd[p + "running_var"][c]) == 0.0 and float(sd[p + "running_mean"][c]) == 0.0


@pytest.mark.parametrize("causal", [False, True])
def test_the_fp32_oracle_is_stressed_but_still_a_yardstick(masks, seeded_sd, coefficients, causal):
    """The largest mask rel_rms of the fp32 oracle over blocks is 2 .. 20 times the seeded rule's on the same input: below that the
    rule stresses nothing, above it E stops being a yardstick.  Measured: 7.6 (offline, 1.98e-6 against 2.61e-7), 4.3 (causal)."""
    def worst(m64, m32):
        return max(float(ref64.rel_err(a, r)[0]) for a, r in zip(m32, m64))
    e_stress = worst(*masks[causal])
    e_seeded = worst(*_masks(seeded_sd, coefficients, causal))
    print(f"largest rel_rms over blocks: stress {e_stress:.3e}, seeded {e_seeded:.3e}, ratio {e_stress / e_seeded:.2f}")
    assert 2.0 <= e_stress / e_seeded <= 20.0, (e_stress, e_seeded)
