"""GPU parity at fp32 rounding: every band of the sliCQT, every block of the CDAE and of the Wiener-EM filter, and the stems,
against the float64 reference (oracle/ref64.py).

Each test computes two errors against ref64 on the same input with the same metric (``ref64.rel_err``: per band or block,
rel_rms = rms(got - ref) / rms(ref), rel_max = max|got - ref| / rms(ref), accumulated in float64):

    e_gpu   the kernels' error                  e_cpu   the fp32 CPU oracle's error (pocketfft / MKL / oneDNN, fp32 throughout)

and asserts  e_gpu <= M * E  for every band / block, where E is the LARGEST e_cpu over the bands or blocks of that stage (the
maximum avoids a band-by-band ratio of two noisy numbers).  M is one number per stage (and one per non-default A/B arm of the
transforms, whose algorithms have other constants): the smallest power of two that is at least twice the worst e_gpu / E
measured on MI355X (the kernels are bitwise deterministic, the factor of two is for another compiler or another box), and it
may not exceed 16 for fp32 and bf16x6 arithmetic.  The measured tables are in
profiles/ref64_parity.json, the worst ratio behind every M in DESIGN.md section 2.  With XSQ_REF64_TABLES=<file> the tables of
a run are written there as JSON.
"""
import numpy as np
import pytest
import torch

from oracle import ref64
from oracle.parity import M_CAP, Tables
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3             # the contractual bar of tests/test_model_gpu.py, kept beside the tight one

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_parity.json).  The stage's M
# holds the default path; an A/B arm whose algorithm has a larger constant has its own, "stage/arm", by the same rule.
M = {
    "forward": 4,                  # 1.92  (n = 9031 impulse, band 261: radix-4 pair-contracted kernel; short_inline is the same code)
    "forward/rocfft": 8,           # 2.72  (n = 650,000 impulse, band 40)
    "forward/dense_bands": 16,     # 6.28  (n = 9031 scaled, band 250: the dense DFT-matrix GEMM sums Lg terms per output in one chain)
    "inverse": 4,                  # 1.003 (n = 9031, all blocks, 7-D)
    "inverse/rocfft": 4,           # 1.93  (n = 70,000, block 46 alone)
    "inverse/dense_bands": 8,      # 2.50  (n = 9031, block 56 alone)
    "cdae": 4,                     # 1.80  fp32 (n = 9031, winograd = 0, block 1), 1.73 bf16x6; bf16x3: 20 .. 31, must fail
    "wiener": 4,                   # 1.02  (masked form, block 1)
    "stems": 4,                    # 1.32  (offline mix-phase, n = 441,000, stem 0)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())

_T = Tables("ref64_parity", M)
_TABLES, _judge = _T.tables, _T.judge


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


@pytest.fixture(scope="module")
def seps():
    from xumx_slicq_amd.separator import seeded_separator
    return {
        "realtime": seeded_separator(realtime=True),
        "offline_phasemix": seeded_separator(realtime=False, wiener=False),
        "offline_wiener": seeded_separator(realtime=False),
    }


def _arm(eng, arm):
    """(set, restore) of one A/B arm of the transform engine."""
    return {"default": (lambda: None, lambda: None),
            "rocfft": (lambda: eng.set_fft_backend(1), lambda: eng.set_fft_backend(0)),
            "dense_bands": (lambda: eng.set_band_radix4(False), lambda: eng.set_band_radix4(True)),
            "short_inline": (lambda: eng.set_short_inline(True), lambda: eng.set_short_inline(False))}[arm]


ARMS = ["default", "rocfft", "dense_bands", "short_inline"]


def _band_labels(plan, rows=None):
    lab = [f"band {j} Lg {int(plan.Lg[j])} {'dense' if plan.Lg[j] < 24 else 'radix4'}" for j in range(plan.nbands)]
    if rows is None:
        return lab
    return [f"row {r} {l}" for r in rows for l in lab]


# ---- forward sliCQT: every band ---------------------------------------------------------------------------------------
def _forward_inputs(plan, n):
    """name -> (x (2, 2, n), per_row).  'synth' keeps every band above 0.5 RMS; 'scaled' has the right channel and batch row 1
    at 1e-3 (relative error is scale-invariant for a linear operator: a cross-channel or cross-row leak of 1e-6 of the loud
    row shows as 1e-3 of the quiet one -- judged per (batch row, channel, band)); 'impulse' puts a unit impulse at the slice
    seams 2h - 1 and 2h, at the last sample in front of the zero-padded tail and at sample 0, one per (row, channel)."""
    x = synth_audio(n, seed=20260101 + n, nb_samples=2)
    scaled = x.clone()
    scaled[:, 1] *= 1e-3
    scaled[1] *= 1e-3
    imp = torch.zeros(2, 2, n)
    h = plan.h
    for r, p in enumerate((2 * h - 1, 2 * h, n - 1, 0)):
        imp[r // 2, r % 2, min(p, n - 1)] = 1.0
    return {"synth": (x, False), "scaled": (scaled, True), "impulse": (imp, True)}


@pytest.mark.parametrize("n", [9031, 70000, 650000])
def test_forward_every_band_is_at_fp32_rounding_of_float64(fb, oracle_plan, n):
    """n = 9031 (S = 3), 70,000 (S = 9) and 650,000 (S = 74), B = 2; bands with Lg < 24 run on the dense grouped GEMM, the
    others on the radix-4 pair-contracted kernel; the default arm and every A/B arm of the engine; (B, 2, n) and (B, 1, 2, n)."""
    from oracle import slicqt as O
    base, enc, dec = fb
    eng, plan = base.nsgt, oracle_plan
    bad = []
    for name, (x, per_row) in _forward_inputs(plan, n).items():
        ref = ref64.forward(plan, x)
        e_cpu = ref64.band_rel_err(O.forward(plan, x), ref, per_row)
        labels = _band_labels(plan, range(4) if per_row else None)
        xd = x.cuda()
        for arm in ARMS:
            on, off = _arm(eng, arm)
            try:
                on()
                C = [c.cpu() for c in enc(xd)]
                C4 = [c.cpu() for c in enc(xd[:, None])] if arm == "default" else None
            finally:
                off()
            assert len(C) == 70 and C[0].shape[3] == plan.nslices(n)
            b, _ = _judge("forward", f"n={n} {name} {arm}", ref64.band_rel_err(C, ref, per_row), e_cpu, labels,
                          full_table=(arm == "default" and name == "synth"), arm=arm)
            bad += [f"n={n} {name} {arm} {m}" for m in b]
            if C4 is not None:
                assert all(c.shape == (2, 1, *r.shape[1:]) for c, r in zip(C4, ref))
                b, _ = _judge("forward", f"n={n} {name} lead (2, 1, 2)", ref64.band_rel_err(C4, [r[:, None] for r in ref], per_row),
                              e_cpu, labels)
                bad += [f"n={n} {name} 4-D input {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- inverse sliCQT: one block at a time ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9031, 70000])
def test_inverse_of_each_block_alone_is_at_fp32_rounding_of_float64(fb, oracle_plan, n):
    """Coefficients that are zero except in ONE block (seeded normal), for each of the 70 blocks -- stacked along a leading
    dimension of 70, so one call decodes them all: in the all-bands tests one wrong dual-window value is 1 / 263 of the energy,
    alone it is all of it.  Then all blocks at once as the 7-D (4, B, 2, ...) input Unmix returns."""
    from oracle import slicqt as O
    base, enc, dec = fb
    eng, plan = base.nsgt, oracle_plan
    S = plan.nslices(n)
    gen = torch.Generator().manual_seed(n)
    P = []
    for k, (_, F, T) in enumerate(plan.blocks):
        p = torch.zeros(70, 1, 2, F, S, T, 2)
        p[k] = torch.randn(1, 2, F, S, T, 2, generator=gen)
        P.append(p)
    gen = torch.Generator().manual_seed(n + 1)
    Q = [torch.randn(4, 2, 2, F, S, T, 2, generator=gen) for (_, F, T) in plan.blocks]
    bad = []
    for tag, X, labels in (("one block", P, [f"block {k} F {F} T {T}" for k, (_, F, T) in enumerate(plan.blocks)]),
                           ("all blocks 7-D", Q, [f"stem {t}" for t in range(4)])):
        ref = ref64.inverse(plan, X, n)
        e_cpu = ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,))
        Xd = [p.cuda() for p in X]
        for arm in ARMS:
            on, off = _arm(eng, arm)
            try:
                on()
                y = dec(Xd, n).cpu()
            finally:
                off()
            assert y.shape == ref.shape
            b, _ = _judge("inverse", f"n={n} {tag} {arm}", ref64.rel_err(y, ref, keep=(0,)), e_cpu, labels, full_table=(arm == "default"), arm=arm)
            bad += [f"n={n} {tag} {arm} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- CDAE: all 70 blocks, both models, pointwise ----------------------------------------------------------------------
def _mask_errors(masks, ref):
    r, m = zip(*(ref64.rel_err(a, b) for a, b in zip(masks, ref)))
    return np.array(r, dtype=np.float64), np.array(m, dtype=np.float64)


def _logit_report(masks, ref, blocks):
    """The layer-4 pre-activation error on the values in (0.02, 0.98) of the named blocks: not flattened by the sigmoid."""
    out = []
    for b in blocks:
        mid = (ref[b] > 0.02) & (ref[b] < 0.98)
        d = (ref64.cdae_logits(masks[b].double().clamp(1e-12, 1 - 1e-12)) - ref64.cdae_logits(ref[b]))[mid].abs()
        out.append(f"block {b}: logit error max {float(d.max()):.3e} rms {float(d.pow(2).mean().sqrt()):.3e} over {int(mid.sum())} values")
    return out


CDAE_ARMS = [("fp32", None), ("fp32", 0), ("fp32", 1), ("fp32", 3), ("fp32", 7), ("bf16x6", None)]


@pytest.mark.parametrize("n,B", [(9031, 2), (395000, 1), (585000, 1)])
@pytest.mark.parametrize("name,causal", [("offline_phasemix", False), ("realtime", True)])
def test_cdae_masks_of_every_block_are_at_fp32_rounding_of_float64(seps, oracle_plan, seeded_sd, name, causal, n, B):
    """ref64 is fed the GPU's own fp32 coefficients, so only the model is under test.  S = 3 (rows shorter than a slab tile),
    S = 45 (layer 2 / 3 rows of 86 / 89 positions: the direct slab kernels at the lower edge of their range) and S = 66 (rows of
    128 / 131 positions: Winograd F(2, 4)); the arms xsq_model_set_winograd 0, 1, 3, 7 and the default, and the
    bf16x6 mode under the same cap.  bf16x3 (opt-in, documented as 10x less accurate) is measured on the same table: it must
    FAIL the bound the fp32 path is held to, which shows that the test resolves a tenfold loss in the default arithmetic."""
    from oracle import model as omodel
    from xumx_slicq_amd import _lib
    sep = seps[name]
    m = sep.xumx_model
    x = synth_audio(n, seed=20260101 + n, nb_samples=B)
    X = sep.nsgt(x.cuda())
    Xc = [b.cpu() for b in X]
    ref = [ref64.cdae_masks(seeded_sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)]
    e_cpu = _mask_errors([omodel.cdae_masks(seeded_sd, b, omodel.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)], ref)
    labels = [f"block {b} F {F} T {T}" for b, (_, F, T) in enumerate(oracle_plan.blocks)]
    bad = []

    def run(precision, wino):
        try:
            m.set_precision(precision)
            if wino is not None:
                m.set_winograd(wino)
            _lib.profile_enable(True)
            _lib.profile_reset()
            _, masks = m(X, return_masks=True)
            masks = [k.cpu() for k in masks]
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
            m.set_precision("fp32")
            m.set_winograd(True)
        print(f"[cdae] {name} n={n} {precision} winograd={wino}: kernels " + ", ".join(f"{k} x{c}" for k, (_, c) in sorted(prof.items())))
        return masks

    for precision, wino in CDAE_ARMS:
        masks = run(precision, wino)
        case = f"{name} n={n} B={B} {precision} winograd={'default' if wino is None else wino}"
        b, _ = _judge("cdae", case, _mask_errors(masks, ref), e_cpu, labels, full_table=(wino is None))
        if b:
            worst = sorted(range(70), key=lambda i: -float((masks[i].double() - ref[i]).abs().max()))[:3]
            bad += [f"{case} {msg}" for msg in b] + _logit_report(masks, ref, worst)
    # the opt-in split-bf16 mode with three products: measured, and it must be VISIBLE to this test
    masks = run("bf16x3", None)
    g = _mask_errors(masks, ref)
    E_rms, E_max = float(e_cpu[0].max()), float(e_cpu[1].max())
    ratio3 = float(np.maximum(g[0] / E_rms, g[1] / E_max).max())
    print(f"[cdae] {name} n={n} bf16x3: worst e_gpu / E = {ratio3:.1f} (fp32 bound: {M['cdae']})")
    _TABLES.setdefault("cdae_bf16x3", {})[f"{name} n={n} B={B}"] = {"M_key": "cdae/bf16x3 (measured; must exceed M of cdae)", "worst_ratio": ratio3, "E_rms": E_rms, "E_max": E_max}
    assert not bad, "\n".join(bad)
    assert ratio3 > M["cdae"], f"bf16x3 passes the fp32 bound ({ratio3:.1f} <= {M['cdae']}): the test cannot see a tenfold loss"


# ---- Wiener-EM: every block -------------------------------------------------------------------------------------------
def test_wiener_em_of_every_block_is_at_fp32_rounding_of_float64(seps, oracle_plan):
    """Real block shapes at n = 150,000 with B = 2 (S = 18): blocks with T >= 280 have a full 5000-frame window followed by a
    short one; batch row 1 is 40 times louder, and the window maximum is shared over the batch.  (a) the masked form the
    separator runs (Unmix.forward: layer 4 stores the masks, the EM passes form mask * X as they load) and (b) the module-level
    ``blockwise_wiener`` on the same initial magnitudes, both against ref64.blockwise_wiener."""
    from oracle import model as omodel
    from xumx_slicq_amd.phase import blockwise_wiener
    n = 150000
    sep = seps["offline_wiener"]
    x = synth_audio(n, seed=20260101 + n, nb_samples=2)
    x[1] *= 40.0
    X = sep.nsgt(x.cuda())
    Y, masks = sep.xumx_model(X, return_masks=True)
    labels = [f"block {b} F {F} T {T} windows {-(-(18 * T) // 5000)}" for b, (_, F, T) in enumerate(oracle_plan.blocks)]
    assert X[0].shape[3] == 18 and any(18 * T > 5000 and (18 * T) % 5000 for (_, F, T) in oracle_plan.blocks)
    g_masked, g_module, c = [], [], []
    for b in range(70):
        Xb, mb = X[b].cpu(), masks[b].cpu()
        ref = ref64.blockwise_wiener(Xb, mb.double() * ref64.abs_of_real_complex(Xb))
        Ymag = mb * omodel.abs_of_real_complex(Xb)                        # fp32, what the oracle and the module call start from
        ref_m = ref64.blockwise_wiener(Xb, Ymag)
        c.append(ref64.rel_err(omodel.blockwise_wiener(Xb, Ymag), ref_m))
        g_masked.append(ref64.rel_err(Y[b], ref))
        g_module.append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda()), ref_m))
    e_cpu = tuple(np.array([float(v[i]) for v in c]) for i in (0, 1))
    bad = []
    for tag, g in (("masked (Unmix.forward)", g_masked), ("blockwise_wiener", g_module)):
        b, _ = _judge("wiener", f"n={n} B=2 {tag}", tuple(np.array([float(v[i]) for v in g]) for i in (0, 1)), e_cpu, labels, full_table=True)
        bad += [f"{tag} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- end to end ---------------------------------------------------------------------------------------------------------
FULL_CHUNK = 2621440


@pytest.mark.parametrize("n", [100000, 441000, FULL_CHUNK + 98240])
@pytest.mark.parametrize("name,causal,wiener", [
    ("realtime", True, False), ("offline_phasemix", False, False), ("offline_wiener", False, True)])
def test_stems_are_at_fp32_rounding_of_float64(seps, oracle_plan, seeded_sd, name, causal, wiener, n):
    """Separator.forward against ref64.separate (chunk by chunk, as the separator cuts the track), per stem: S = 13, S = 50, and
    one full chunk (S = 292: 18 Wiener windows in block 69, each with its own maximum) followed by the 98,240-sample tail chunk.
    The contractual 1e-4 RMS / 1e-3 max-abs bar is asserted beside the tight one."""
    from oracle import separator as osep
    sep = seps[name]
    sep.chunk_size = FULL_CHUNK
    x = synth_audio(n, seed=20260101 + n)
    est = sep(x.cuda()).cpu()
    ref = torch.cat([ref64.separate(oracle_plan, seeded_sd, x[..., p:p + FULL_CHUNK], causal=causal, wiener=wiener)
                     for p in range(0, n, FULL_CHUNK)], dim=-1)
    orc = osep.separate(oracle_plan, seeded_sd, x, causal=causal, wiener=wiener)
    assert est.shape == ref.shape == (4, 1, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (name, n, rms, mx)
    bad, _ = _judge("stems", f"{name} n={n}", ref64.rel_err(est, ref, keep=(0,)), ref64.rel_err(orc, ref, keep=(0,)),
                    [f"stem {t}" for t in range(4)], full_table=True)
    assert not bad, "\n".join(bad)
