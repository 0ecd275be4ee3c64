"""Layers 2 and 3 of the one-tap CDAE blocks in one launch (csrc/cdae_wino23.h, bit 16 of xsq_model_set_winograd, on by default) against
the two Winograd F(2, 4) launches it replaces (``set_winograd(7)``): the masks of all 70 blocks BIT FOR BIT, no tolerance -- every value
goes through the same operations in the same order, only act2 stays in LDS.

A fused tile is 62 act3 pairs of one row, computed from 64 act2 pairs (two pairs of halo on the left).  The fusion applies where BOTH
layers run F(2, 4): ``(T2 + 1) // 2 >= 64`` with T2 = T1 - 3, T1 = 2 S - 1 offline and 2 S causal, i.e. S >= 66 offline and S >= 65 causal.
Shapes (B = 2):
  S = 66   the smallest offline shape that fuses: T1 = 131, 66 act3 pairs per row = one full tile and a 4-pair remainder
  S = 67, 68  the odd and even ends of a row beside it (the causal rows have even T1, the offline rows odd T1), act2's zero padding at
           both row ends
  S = 125  offline 125 pairs per row: three tiles, the seams at pairs 62 and 124 and their two-pair halo; causal the same three tiles
  S = 65   causal: its smallest fusing shape (T2 = 127).  Offline: layer 3 runs F(2, 4), layer 2 the direct slab kernel -- nothing fuses and
           the launch counts are those of mask 7.
The profile counters: the fused launch is one launch under each of ``cdae_l2_slab`` and ``cdae_l3_slab`` (half of its time each), the
multi-tap blocks keep a launch of their own per layer -- two launches per name on Bark-262, the name set unchanged."""
import pytest
import torch

from test_ref64_sweep_cpu import n_of
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu

DEFAULT_MASK, UNFUSED_MASK = 23, 7
B = 2


@pytest.fixture(scope="module")
def seps():
    from xumx_slicq_amd.separator import seeded_separator
    return {"realtime": seeded_separator(realtime=True), "offline_phasemix": seeded_separator(realtime=False, wiener=False)}


def fuses(causal, S):
    T1 = 2 * S if causal else 2 * S - 1
    return (T1 - 3 + 1) // 2 >= 64


def _run(m, X, mask):
    """Masks of every block and the CDAE layers' launch counts under ``mask`` (None: whatever the model has, i.e. the default)."""
    from xumx_slicq_amd import _lib
    try:
        if mask is not None:
            m.set_winograd(mask)
        _lib.profile_enable(True)
        _lib.profile_reset()
        _, masks = m(X, return_masks=True)
        masks = [k.cpu() for k in masks]
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
        m.set_winograd(True)
    return masks, {k: int(c) for k, (_, c) in prof.items() if k.startswith("cdae_l")}


CASES = [(name, causal, S) for name, causal in (("offline_phasemix", False), ("realtime", True)) for S in (66, 67, 68, 125)] + \
        [("realtime", True, 65), ("offline_phasemix", False, 65)]


def test_the_cases_cover_both_sides_of_the_threshold():
    assert [fuses(c, S) for _, c, S in CASES] == [True] * 9 + [False]
    assert not fuses(True, 64) and not fuses(False, 65) and fuses(False, 66) and fuses(True, 65)


@pytest.mark.parametrize("name,causal,S", CASES, ids=[f"{name}-S{S}" for name, _, S in CASES])
def test_fused_layers_2_and_3_give_the_two_launches_masks_bit_for_bit(seps, name, causal, S):
    sep = seps[name]
    m = sep.xumx_model
    assert int(getattr(m, "winograd", DEFAULT_MASK)) == DEFAULT_MASK
    X = sep.nsgt(synth_audio(n_of(S), seed=20261020 + S, nb_samples=B).cuda())
    assert len(X) == 70 and X[0].shape[0] == B and X[0].shape[3] == S
    try:
        fused, launches = _run(m, X, None)
        explicit, launches_explicit = _run(m, X, DEFAULT_MASK)
        plain, launches_plain = _run(m, X, UNFUSED_MASK)
    finally:
        m.set_winograd(True)
    assert int(m.winograd) == DEFAULT_MASK
    assert all(bool(torch.isfinite(k).all()) for k in fused)
    differ = [b for b in range(70) if not torch.equal(fused[b], plain[b])]
    assert not differ, f"{name} S={S}: blocks {differ} differ from set_winograd({UNFUSED_MASK})"
    assert all(torch.equal(a, b) for a, b in zip(fused, explicit)) and launches == launches_explicit
    print(f"[fused23] {name} S={S}: default {launches}, mask {UNFUSED_MASK} {launches_plain}")
    assert set(launches) == set(launches_plain), (launches, launches_plain)
    assert {"cdae_l3_slab"} <= set(launches)
    if fuses(causal, S):
        assert launches["cdae_l2_slab"] == 2 and launches["cdae_l3_slab"] == 2, launches
        assert launches_plain["cdae_l2_slab"] == 1 and launches_plain["cdae_l3_slab"] == 1, launches_plain
        assert {k: c for k, c in launches.items() if not k.endswith("_slab")} == {k: c for k, c in launches_plain.items() if not k.endswith("_slab")}
    else:
        assert launches == launches_plain, (launches, launches_plain)
