"""Why the shapes of tests/test_ref64_sweep_gpu.py are enough: the case lists of that module, and, restated on the host, what each
case selects in the library -- the kernel class of layers 2 / 3 from the row length, the tile tails and item crossings of the pair-tiled
kernels, the row tiles of the radix-4 band kernels, the 5000-frame windows of the Wiener-EM filter.  No GPU.  The tests fail if someone
trims a list.

Kernel choice (csrc/cdae.hip, ``cdae_launch_layer``): layer 3 has rows of ``T1`` positions (``2S - 1`` offline, ``2S`` causal), layer 2 of
``T2 = T1 - 3``; below 86 the grouped GEMM runs, from 86 the direct slab kernel, from 127 (64 output pairs) Winograd F(2, 4).  The profile
counters name the launch site: ``cdae_l2_slab`` / ``cdae_l3_slab`` for both slab classes, ``cdae_l2_gemm`` / ``cdae_l3_gemm`` below.

Tiles of 64 output pairs (``get_l1f_tiles``, ``get_l4f_tiles``: (b, f, pair) flattened over the batch; ``get_wino_tiles``: per item):
an item holds ``Fo * P`` pairs, so ``Fo * P mod 64`` is the tail of an item's last tile and, for the flattened tables, ``i * Fo * P mod 64``
is where item ``i`` starts inside a tile.  With ``P = S`` a multiple of 64 (S = 64 and S = 128) every item starts on a tile: those two cases
are the tail-free extreme, every other case has an item boundary inside a tile in every block.

The one slow check (19 to 25 s on an 8-thread host) is the condition on E of the GPU module: E there is the largest fp32-oracle error over ``E_BLOCKS`` instead of all
70 blocks, and that subset has to carry at least 0.75 of the all-block E on the module's own synth input at S = 66, B = 3.  It is computed
for the offline model only (the fp32 oracle takes 16 to 22 s for the 70 blocks of one model); measured for both when the subset was chosen:
1.00 / 1.00 offline and causal, block 1 (F 86, kf 5) is the arg-max of both metrics in both, blocks 3 and 27 follow at 0.84 / 0.73.
"""
import numpy as np
import pytest
import torch

H = 4515                                   # hop of Bark-262 (L = 18060): S slices from n in ((2S - 3) H, (2S - 2) H]
GEMM, SLAB, F24 = "gemm", "slab", "f24"
SLAB_MIN, F24_MIN = 86, 127                # cdae_launch_layer: To >= 86 slab kernels, (To + 1) / 2 >= 64 Winograd F(2, 4)
PAIRS = 64                                 # LF_PAIRS = L4_PAIRS = WN_PAIRS
D4H_ROWS = 32                              # row tile of the radix-4 band kernels
WIN = 5000

# ---- part 1: CDAE cases (model name, causal, S, B) -------------------------------------------------------------------------------
OFFLINE = [(43, 2), (44, 2), (45, 2), (63, 2), (64, 2), (65, 2), (66, 2), (66, 3), (97, 2), (128, 2)]
CAUSAL = [(42, 2), (43, 2), (44, 2), (45, 2), (63, 2), (64, 2), (65, 2), (65, 3)]
CDAE_CASES = [("offline_phasemix", False, S, B) for S, B in OFFLINE] + [("realtime", True, S, B) for S, B in CAUSAL]
# E of a CDAE case: the largest fp32-oracle error over these blocks (1: F 86, kf 5; 2, 3: kf 3; the others kf 1)
E_BLOCKS = (0, 1, 2, 3, 11, 24, 27, 33, 62, 66, 69)

# ---- part 2: transforms (B, S) ------------------------------------------------------------------------------------------------------
FORWARD_CASES = [(1, 3), (1, 16), (1, 17), (3, 11), (2, 64), (5, 13)]          # rows = 2 B S
FORWARD_SCALED = [(3, 11), (5, 13)]
INVERSE_CASES = [(1, 4), (1, 16), (3, 11), (2, 33)]                           # rows = 4 * B * 2 * S
INVERSE_ONE_BLOCK_S = [16, 17]                                                # rows = 70 * 2 * S

# ---- part 3: Wiener-EM (S, B, judged blocks or None = all) ------------------------------------------------------------------------
WIENER_CASES = [(25, 3), (50, 2), (139, 1)]


def n_of(S):
    """A sample count that gives S slices and is no multiple of anything."""
    return (2 * S - 2) * H - 977


def kf_of(F):
    return 1 if F < 10 else (3 if F < 20 else 5)


def rows_of(causal, S):
    """(T1, T2): positions per row of layer 3 / layer 2."""
    T1 = 2 * S if causal else 2 * S - 1
    return T1, T1 - 3


def kernel_class(causal, S, layer):
    T1, T2 = rows_of(causal, S)
    To = T2 if layer == 2 else T1
    return GEMM if To < SLAB_MIN else (SLAB if To < F24_MIN else F24)


def site_names(causal, S):
    """The profile names of the four CDAE layers of a case."""
    return {"cdae_l1_gemm", "cdae_l4_gemm"} | {f"cdae_l{l}_{'gemm' if kernel_class(causal, S, l) == GEMM else 'slab'}" for l in (2, 3)}


def runs_f24(causal, S):
    return F24 in (kernel_class(causal, S, 2), kernel_class(causal, S, 3))


def wiener_windows(S, T):
    """(number of windows, frames of the last one) of a block's S * T frames."""
    N = S * T
    return -(-N // WIN), N - (-(-N // WIN) - 1) * WIN


def wiener_blocks(plan, S):
    """The blocks judged at S: all, except at S = 139 those within 600 frames of one window and the last one."""
    if S != 139:
        return list(range(len(plan.blocks)))
    return [b for b, (_, F, T) in enumerate(plan.blocks) if abs(S * T - WIN) <= 600] + [len(plan.blocks) - 1]


@pytest.fixture(scope="module")
def shapes(oracle_plan):
    assert oracle_plan.h == H and len(oracle_plan.blocks) == 70
    out = []
    for _, F, T in oracle_plan.blocks:
        kf = kf_of(F)
        out.append((F, T, kf, F - kf + 1, F - 2 * kf + 2))                      # F, T, kf, F1, F2
    return out


def test_n_of_gives_the_slices(oracle_plan):
    for S in sorted({S for _, _, S, _ in CDAE_CASES} | {S for _, S in FORWARD_CASES + INVERSE_CASES} | set(INVERSE_ONE_BLOCK_S)
                    | {S for S, _ in WIENER_CASES}):
        assert oracle_plan.nslices(n_of(S)) == S and n_of(S) % 2 == 1, S


def test_every_threshold_of_every_layer_is_met_from_both_sides():
    """For each model, layer and threshold the list holds the largest S below it and the smallest S at or above it."""
    for causal in (False, True):
        have = {S for _, c, S, _ in CDAE_CASES if c == causal}
        for layer in (2, 3):
            for below, above in ((GEMM, SLAB), (SLAB, F24)):
                lo = max(S for S in range(3, 200) if kernel_class(causal, S, layer) == below)
                assert kernel_class(causal, lo + 1, layer) == above
                assert lo in have and lo + 1 in have, (causal, layer, below, above, lo)
                print(f"{'causal' if causal else 'offline'} layer {layer}: {below} at S = {lo} (To = {rows_of(causal, lo)[layer == 2]}), "
                      f"{above} at S = {lo + 1} (To = {rows_of(causal, lo + 1)[layer == 2]})")


def test_every_mixed_case_is_present():
    """Layer 3 one class ahead of layer 2: slab over GEMM at S = 44 offline and S = 43, 44 causal; F(2, 4) over slab at S = 64, 65 offline
    and S = 64 causal.  And nothing else in the lists is mixed."""
    mixed = {(c, S): (kernel_class(c, S, 2), kernel_class(c, S, 3)) for _, c, S, _ in CDAE_CASES
             if kernel_class(c, S, 2) != kernel_class(c, S, 3)}
    assert mixed == {(False, 44): (GEMM, SLAB), (True, 43): (GEMM, SLAB), (True, 44): (GEMM, SLAB),
                     (False, 64): (SLAB, F24), (False, 65): (SLAB, F24), (True, 64): (SLAB, F24)}
    # the site names the GPU module asserts, on the issue's own examples
    assert site_names(False, 44) == {"cdae_l1_gemm", "cdae_l2_gemm", "cdae_l3_slab", "cdae_l4_gemm"}
    assert not any(n.endswith("slab") for n in site_names(False, 43))
    # the direct slab kernel's fourth segment: a 256-row tile touches four rows only where 86 <= To <= 127
    assert any(SLAB_MIN <= To <= 127 and kernel_class(c, S, l) == SLAB for _, c, S, _ in CDAE_CASES for l, To in zip((3, 2), rows_of(c, S)))
    # F(2, 4) against the direct kernel by bits: the lists hold cases on both sides for both models
    for causal in (False, True):
        assert {runs_f24(c, S) for _, c, S, _ in CDAE_CASES if c == causal} == {False, True}
    assert max(S for _, c, S, _ in CDAE_CASES if not c and not runs_f24(c, S)) == 63
    # the two B = 3 cases: every layer on its long-row kernel
    assert [(c, S) for _, c, S, B in CDAE_CASES if B == 3] == [(False, 66), (True, 65)]
    assert all(kernel_class(c, S, l) == F24 for c, S in ((False, 66), (True, 65)) for l in (2, 3))


def test_tile_tails_and_item_crossings(shapes):
    """``Fo * P mod 64`` over the 70 blocks and the cases: the tails of the pair-tiled kernels.  Layer 1 / 4 as F(2, 2) (offline, P = S,
    Fo = F1 / F), layers 2 / 3 as F(2, 4) (both models, P = ceil(To / 2), Fo = F2 / F1) where the case selects it."""
    tails = {"l1f": set(), "l4f": set(), "f24": set()}
    for _, causal, S, B in CDAE_CASES:
        T1, T2 = rows_of(causal, S)
        for F, T, kf, F1, F2 in shapes:
            if not causal:
                tails["l1f"].add(F1 * S % PAIRS)
                tails["l4f"].add(F * S % PAIRS)
            for layer, To, Fo in ((2, T2, F2), (3, T1, F1)):
                if kernel_class(causal, S, layer) == F24:
                    tails["f24"].add(Fo * ((To + 1) // 2) % PAIRS)
    union = set().union(*tails.values())
    print("distinct Fo * P mod 64:", {k: len(v) for k, v in tails.items()}, "union", len(union))
    assert len(union) >= 32 and all(len(v) >= 32 for v in tails.values())
    assert 0 in tails["l1f"] and 0 in tails["l4f"] and 0 in tails["f24"]                 # ... and the tail-free tile

    # an item boundary inside a tile of the flattened (b, f, pair) tables (offline model: layers 1 and 4)
    aligned = []
    for _, causal, S, B in CDAE_CASES:
        if causal or B < 2:
            continue
        for name, idx in (("l1f", 3), ("l4f", 0)):
            crossing = sum(any(i * sh[idx] * S % PAIRS for i in range(1, B)) for sh in shapes)
            if S % PAIRS == 0:
                assert crossing == 0, (S, B, name)
                aligned.append(S)
            else:
                assert 2 * crossing >= len(shapes), (S, B, name, crossing)
    # S = 128 is the chosen tail-free extreme; S = 64 is one too, by the same arithmetic (P = S = 64: every Fo * P is a multiple of 64)
    assert sorted(set(aligned)) == [64, 128]
    assert all(B >= 2 for _, _, _, B in CDAE_CASES)

    # the run partition of layer 4 (L4F_RUN = 6, one-tap blocks): rtiles * r / nruns over many more rtiles than before, runs of every
    # length 2 .. 6 (the smallest block has two row tiles), and partitions whose runs are not all equal
    runs, uneven, seen = set(), 0, set()
    for _, causal, S, B in CDAE_CASES:
        if causal:
            continue
        for F, T, kf, F1, F2 in shapes:
            if kf != 1:
                continue
            rtiles = -(-B * F * S // PAIRS)
            nruns = -(-rtiles // 6)
            lens = {rtiles * (r + 1) // nruns - rtiles * r // nruns for r in range(nruns)}
            assert sum(rtiles * (r + 1) // nruns - rtiles * r // nruns for r in range(nruns)) == rtiles and max(lens) <= 6 and min(lens) >= 1
            runs |= lens
            uneven += len(lens) > 1
            seen.add(rtiles)
    print(f"layer-4 run partition: {len(seen)} distinct rtiles, run lengths {sorted(runs)}, {uneven} uneven partitions")
    assert runs == {2, 3, 4, 5, 6} and uneven >= 10 and len(seen) >= 20, (runs, uneven, len(seen))


def test_row_counts_of_the_transform_cases():
    fwd = [2 * B * S for B, S in FORWARD_CASES]
    inv = [8 * B * S for B, S in INVERSE_CASES]
    assert fwd == [6, 32, 34, 66, 256, 130] and inv == [32, 128, 264, 528]
    assert any(r < D4H_ROWS for r in fwd) and D4H_ROWS in fwd and D4H_ROWS in inv
    assert sum(r % D4H_ROWS == 2 for r in fwd) >= 3 and any(r % 256 == 0 for r in fwd) and any(r > 512 for r in inv)
    assert any(r % D4H_ROWS == 0 and r > D4H_ROWS for r in inv) and any(r % D4H_ROWS not in (0, 2) for r in inv)
    assert [70 * 2 * S % D4H_ROWS for S in INVERSE_ONE_BLOCK_S] == [0, 12]
    assert set(FORWARD_SCALED) <= set(FORWARD_CASES) and all(B >= 3 for B, _ in FORWARD_SCALED)


def test_wiener_window_coincidences(oracle_plan):
    """Each named S * T coincidence exists in the plan."""
    T = [t for _, _, t in oracle_plan.blocks]
    w = {S: [wiener_windows(S, t) for t in T] for S, _ in WIENER_CASES}
    assert (1, WIN) in w[25] and (2, 100) in w[25] and any(k == 1 and tail < WIN for k, tail in w[25])            # T = 200, 204, <= 196
    assert (1, WIN) in w[50] and (2, WIN) in w[50] and (2, 200) in w[50]                                         # T = 100, 200, 104
    assert (2, 4) in w[139]                                                                                      # T = 36
    assert 25 * 200 == WIN and 25 * 204 == WIN + 100 and 50 * 100 == WIN and 50 * 200 == 2 * WIN and 50 * 104 == WIN + 200 and 139 * 36 == WIN + 4
    assert 200 in T and 204 in T and 196 in T and 100 in T and 104 in T and 36 in T
    judged = wiener_blocks(oracle_plan, 139)
    assert [T[b] for b in judged] == [32, 36, 40, 292] and len(wiener_blocks(oracle_plan, 25)) == 70
    assert max(k for k, _ in w[139]) == 9 and [B for _, B in WIENER_CASES] == [3, 2, 1]


def test_the_block_subset_carries_the_oracle_error(oracle_plan, seeded_sd):
    """E of the GPU module's CDAE cases is the largest fp32-oracle error over ``E_BLOCKS``; at S = 66, B = 3 on that module's synth input it
    is at least 0.75 of the all-block E in both metrics.  Offline model only (see the module docstring)."""
    from oracle import model as omodel
    from oracle import ref64
    from oracle import slicqt as O
    from xumx_slicq_amd.synth import synth_audio
    assert 1 in E_BLOCKS and {24, 62, 66} <= set(E_BLOCKS) and 9 <= len(E_BLOCKS) <= 12
    kfs = {kf_of(oracle_plan.blocks[b][1]) for b in E_BLOCKS}
    assert kfs == {1, 3, 5} and oracle_plan.blocks[1][1:] == (86, 16)
    S, B = 66, 3
    n = n_of(S)
    X = O.forward(oracle_plan, synth_audio(n, seed=20260101 + n, nb_samples=B))
    assert X[0].shape[3] == S
    e = []
    with torch.no_grad():
        for b, Xb in enumerate(X):
            ref = ref64.cdae_masks(seeded_sd, b, ref64.abs_of_real_complex(Xb), False)
            e.append([float(v) for v in ref64.rel_err(omodel.cdae_masks(seeded_sd, b, omodel.abs_of_real_complex(Xb), False), ref)])
    e = np.array(e)
    share = e[list(E_BLOCKS)].max(0) / e.max(0)
    print(f"offline S = {S} B = {B}: all-block E_rms {e[:, 0].max():.3e} E_max {e[:, 1].max():.3e} at blocks {e.argmax(0).tolist()}; "
          f"subset share {share[0]:.3f} / {share[1]:.3f}")
    assert (share >= 0.75).all(), share
