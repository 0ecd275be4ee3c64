"""GPU parity at fp32 rounding on plans other than the two shipped ones: every band of the sliCQT, both adjoints, every block of the
CDAE and of the Wiener-EM filter, the stems and one training step, against the float64 reference (oracle/ref64.py).  Rule, metric and
helpers are those of tests/test_ref64_gpu.py and tests/test_ref64_mel_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err``, E the LARGEST
fp32-oracle error over the members of the stage on the same input, M per stage a power of two, the smallest that is at least twice
the worst e_gpu / E measured on MI355X, at most ``M_CAP``.  The measured tables are in profiles/ref64_plans_parity.json;
tests/test_ref64_plans_cpu.py pins the reference, the plan facts, the floors, and owns the plans and cases.

The plans (tests/test_ref64_plans_cpu.py):  W = ``bark, 400, 300`` (L 27496 on rocFFT, the longest slice that has run; band 0 of
Lg 376, above the 320 of the radix-4 band kernels (its analysis runs on k_band_fwd_long), a block of its own; five-tap blocks (115, 16) and (22, 20); three-tap blocks
(19, 24) .. (10, 44), which turn layer 4's F(2, 2) off for the whole model) and M = ``mel, 64, 115.5`` (L 4096; first blocks (1, 20),
(16, 16)).  T = ``bark, 28, 32.9`` and K = ``bark, 56, 32.9`` have bands that reach across DC, whose mirrored synthesis in the
reference's inverse the kernels do not compute: the library refuses them, and that refusal is what this module asserts of them.

CDAE arms, measured: on W (offline, S = 3 and 66) ``set_winograd(3)`` and ``set_winograd(7)`` return the default's masks BIT FOR BIT
(arm 3 differs from the default by the layer-4 bit, which ``l4f_fits`` turns off on this plan) and arms 0 and 1 differ; on M (offline)
arms 0, 1 and 3 differ; the causal models at S = 3 are bitwise the default on every arm (rows too short to select one), and W causal at
S = 65 differs on arm 0 alone.  The sites of the S = 66 / 65 cases are cdae_l2_slab and cdae_l3_slab (asserted).

Wall time of the module on MI355X: 24 .. 26 s for its 32 tests in one process (the slowest, the forward transform of W with the first
rocFFT plans of L = 27496, 2.4 s; the Wiener-EM filter of W at S = 66 and each CDAE case of W 2.1 .. 2.4 s).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64
from oracle import separator as osep
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables
import test_ref64_train_gpu as TG
from test_autograd_cpu import F32, autograd_forward_adjoint, forward_adjoint_closed_form, random_cotangents
from test_ref64_gpu import CDAE_ARMS, _forward_inputs, _logit_report, _mask_errors
from test_ref64_mel_cpu import one_block_inputs, one_thread, stems_ref, windows
from test_ref64_plans_cpu import (FACTS, GPU_PLANS, LONG_E_BLOCKS, PLANS, REFUSED, SEED, STEM_MODELS, TRAIN_MODELS, audio, kf_of, l4f_fits, make_plan,
                                  make_sd, n_for, train_inputs, train_seed_base)
from test_sdr_cpu import adjoint_closed_form, adjoint_window, autograd_adjoint

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3             # the contractual bar, kept beside the tight one

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_plans_parity.json)
M = {
    "forward": 4,                  # 1.37  (W synth, band 67, Lg 16: rocFFT at L = 27496 + the dense engine's short bands)
    "forward/dense_bands": 16,     # 4.40  (W scaled, row 3, band 400, Lg 260: the dense GEMM sums 2 Lg terms per output in one chain)
    "forward_band0": 4,            # 1.39  (W impulse, row 1, band 0, Lg 376; 1.17 scaled, 1.19 synth); 22.07 on the tile engine, see the test
    "forward_band0/dense_bands": 4,    # 1.39  (the same kernel, k_band_fwd_long, runs this band on both arms)
    "inverse": 8,                  # 2.02  (W, block 0 alone, T 376)
    "inverse/dense_bands": 8,      # 2.14  (M, block 36 alone, T 216)
    "fwd_adjoint": 4,              # 1.78  (W, BC 3, cotangent in bands 0, 1 and 400: row 0)
    "adjoint": 4,                  # 1.33  (W, BC 3: block 1, F 115, T 16)
    "cdae": 4,                     # 1.67  (M offline, S = 3, bf16x6: block 1, F 16, T 16); fp32 arms 1.54; bf16x3: 16.4 .. 44, must fail
    "wiener": 2,                   # 0.91  (M, S = 3, blockwise_wiener, block 1)
    "stems": 4,                    # 1.43  (M, realtime, three chunks, stem 0)
}
# the training step is judged with the M of tests/test_ref64_train_gpu.py; measured here: train/conv 2.07 (M, offline + Wiener, block 0 /
# target 0, 9.weight), train/bn 2.46 (W, causal, block 61), train/whiten 1.98 (W, causal), train/loss 2.22 (W, offline + Wiener),
# train/bn_running 1.39 (W, offline + Wiener, block 61)
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())

_T = Tables("ref64_plans_parity", {**{k: v for k, v in TG.M.items() if k != "train/adamw"}, **M})
_TABLES, _judge = _T.tables, _T.judge
ARMS = ["default", "dense_bands"]


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    import time
    t0 = time.time()
    yield
    _T.record("wall_s", "module", {"M_key": "wall_s (seconds from the first test's setup to the last one's end; not judged)", "worst_ratio": 0.0,
                                   "seconds": time.time() - t0})
    _T.dump()


_FB, _SEPS = {}, {}


def _fb(name):
    if name not in _FB:
        from xumx_slicq_amd.transforms import NSGTBase, make_filterbanks
        base = NSGTBase(*PLANS[name], device="cuda")
        _FB[name] = (base, *make_filterbanks(base))
    return _FB[name]


def _sep(name, model):
    if (name, model) not in _SEPS:
        from xumx_slicq_amd.separator import seeded_separator
        cfg = dict(fscale=PLANS[name][0], fbins=PLANS[name][1], fmin=PLANS[name][2], seed=SEED)
        kw = {"realtime": dict(realtime=True), "offline_phasemix": dict(realtime=False, wiener=False), "offline_wiener": dict(realtime=False)}[model]
        _SEPS[name, model] = seeded_separator(**kw, **cfg)
    return _SEPS[name, model]


@pytest.fixture(scope="module", autouse=True)
def _drop_graphs():
    yield
    for s in _SEPS.values():
        s.drop_graphs()
    _SEPS.clear()
    _FB.clear()


def _arm(eng, arm):
    return {"default": (lambda: None, lambda: None),
            "dense_bands": (lambda: eng.set_band_radix4(False), lambda: eng.set_band_radix4(True))}[arm]


def _block_labels(plan, S=None):
    return [f"block {b} F {F} T {T}" + ("" if S is None else f" windows {windows(S, T)[0]}") for b, (_, F, T) in enumerate(plan.blocks)]


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


# ---- the plans the library refuses ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(REFUSED))
def test_plans_with_a_band_across_dc_are_refused(name):
    """NSGTBase, and with it build_models, Separator and the training entry point, raise before any table reaches the device, naming
    the band (xsq_plan_create's own refusal is asserted in tests/test_ref64_plans_cpu.py: it needs no device)."""
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.transforms import NSGTBase
    with pytest.raises(ValueError, match=rf"band {REFUSED[name]} .*reaches across DC"):
        NSGTBase(*PLANS[name], device="cuda")
    with pytest.raises(ValueError, match="reaches across DC"):
        seeded_separator(realtime=True, fscale=PLANS[name][0], fbins=PLANS[name][1], fmin=PLANS[name][2], seed=SEED)


# ---- forward sliCQT: every band ------------------------------------------------------------------------------------------------------
_FORWARD = {}


def _forward_failures(name):
    """stage -> failures of the forward transform of plan ``name``; computed once, both tests below read it."""
    if name in _FORWARD:
        return _FORWARD[name]
    base, enc, dec = _fb(name)
    eng, plan = base.nsgt, make_plan(name)
    n = n_for(plan, 3)
    bad = {"forward": [], "forward_band0": []}
    for inp, (x, per_row) in _forward_inputs(plan, n).items():
        ref = ref64.forward(plan, x)
        e_cpu = ref64.band_rel_err(O.forward(plan, x), ref, per_row)
        rows = range(4) if per_row else [None]
        labels = [(f"row {r} " if r is not None else "") + f"band {j} Lg {int(plan.Lg[j])}" for r in rows for j in range(plan.nbands)]
        own = np.array([name == "W" and j == 0 for _ in rows for j in range(plan.nbands)])
        xd = x.cuda()
        for arm in ARMS:
            on, off = _arm(eng, arm)
            try:
                on()
                C = [c.cpu() for c in enc(xd)]
            finally:
                off()
            assert len(C) == len(plan.blocks) and C[0].shape[3] == 3
            e_gpu = ref64.band_rel_err(C, ref, per_row)
            for stage, sel in (("forward", ~own), ("forward_band0", own)):
                if sel.any():
                    b, _ = _judge(stage, f"{name} {inp} {arm}", tuple(e.reshape(-1)[sel] for e in e_gpu), tuple(e.reshape(-1)[sel] for e in e_cpu),
                                  [l for l, s in zip(labels, sel) if s], full_table=(arm == "default" and inp == "synth"), arm=arm)
                    bad[stage] += [f"{name} {inp} {arm} {m}" for m in b]
    _FORWARD[name] = bad
    return bad


@pytest.mark.parametrize("name", GPU_PLANS)
def test_forward_every_band_is_at_fp32_rounding_of_float64(name):
    """S = 3, B = 2; 'synth', 'scaled' and 'impulse' (tests/test_ref64_gpu.py); the default arm (rocFFT + radix-4 band kernels) and every
    band up to Lg 320 on the dense GEMM.  Every band but band 0 of W, which has the test below."""
    bad = _forward_failures(name)["forward"]
    assert not bad, "\n".join(bad)


def test_forward_of_the_lg_376_band_of_w_is_at_fp32_rounding_of_float64():
    """Band 0 of W (Lg 376, above the 320 of the radix-4 band kernels, so the same kernel on both arms), judged under a stage of its
    own on the same three inputs.

    This test found a defect, since fixed.  On the dense DFT-matrix GEMM (gemm_tile.h), where every band above Lg 320 ran, the worst
    e_gpu / E was 5.47 (synth), 5.99 (scaled, row 3) and 22.07 (impulse, rows 1 and 3: the impulses at the slice seam 2h and at
    sample 0; e_gpu rms 2.85e-6, max 1.35e-4 against E_rms 2.98e-7, E_max 6.1e-6): above M_CAP.  Cause: that engine sums the
    K = 2 Lg = 752 products of an output in ONE fp32 MFMA accumulator chain.  The DC window is a plateau of ones with Hann edges, and
    an impulse at a slice seam has a spectrum of constant modulus, so at the coefficient where the phases align the 361 plateau terms
    add with one sign and the chain's rounding grows with the term count (7e-6 of that coefficient), where the oracle's FFT grows with
    its logarithm.  (Blackman-Harris bands taper: Lg 200 .. 292 on the same engine stay at 3 .. 5.4, the `forward/dense_bands`
    stage.)  The analysis of such bands now runs on k_band_fwd_long (csrc/slicqt.hip), which carries the sum in float64 and rounds
    once: 1.19 / 1.17 / 1.39 on the three inputs.  Plans with no band above Lg 320 (Bark-262, Mel-32, M) launch what they did."""
    bad = _forward_failures("W")["forward_band0"]
    assert not bad, "\n".join(bad)


# ---- inverse sliCQT: one block at a time, and against the reference's own decode -------------------------------------------------
@pytest.mark.parametrize("name", GPU_PLANS)
def test_inverse_of_each_block_alone_is_at_fp32_rounding_of_float64(name):
    """Coefficients that are zero except in ONE block, for each block, stacked along a leading dimension so one call decodes them
    all; then all blocks at once as the 7-D (4, B, 2, ...) input Unmix returns."""
    base, enc, dec = _fb(name)
    eng, plan = base.nsgt, make_plan(name)
    n = n_for(plan, 3)
    P, Q = one_block_inputs(plan, n)
    bad = []
    for tag, X, labels in (("one block", P, _block_labels(plan)), ("all blocks 7-D", Q, [f"stem {t}" for t in range(4)])):
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
            b, _ = _judge("inverse", f"{name} {tag} {arm}", ref64.rel_err(y, ref, keep=(0,)), e_cpu, labels, full_table=(arm == "default"), arm=arm)
            bad += [f"{name} {tag} {arm} {m}" for m in b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", GPU_PLANS)
def test_transforms_equal_the_reference_fixture(name):
    """The reference's own numbers (tests/golden/plans3_<name>.npz): forward coefficients at 2e-5 (the bound of tests/test_mel_plan.py),
    and the waveform decoded from all blocks and from BLOCK 0 ALONE at the contractual 1e-4 RMS / 1e-3 max-abs."""
    base, enc, dec = _fb(name)
    plan, g = make_plan(name), load_golden(f"plans3_{name}.npz")
    n = int(g["n"])
    from xumx_slicq_amd.synth import synth_audio
    C = enc(synth_audio(n, seed=20260101 + n).cuda())
    for i, cb in enumerate(C):
        if f"fwd_{i}" in g:
            assert float((cb.cpu() - torch.from_numpy(g[f"fwd_{i}"])).abs().max()) < 2e-5, (name, i)
    for key, X in (("inv", C), ("inv_block0", [c if i == 0 else torch.zeros_like(c) for i, c in enumerate(C)])):
        d = dec(X, n).cpu().double() - torch.from_numpy(g[key]).double()
        rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
        print(f"[fixture] {name} {key}: GPU decode against the reference's: rms {rms:.2e} max {mx:.2e}")
        _T.record("fixture", f"{name} {key}", {"M_key": "fixture (absolute distance from the reference's decode; bar 1e-4 RMS / 1e-3 max)", "worst_ratio": mx / MAX_TOL,
                                               "rms": rms, "max": mx})
        assert rms < RMS_TOL and mx < MAX_TOL, (name, key, rms, mx)


# ---- both adjoints --------------------------------------------------------------------------------------------------------------------
def _edge_bands_only(plan, G):
    keep = {0, 1, plan.nbands - 1}
    for (j0, F, T), g in zip(plan.blocks, G):
        for f in range(F):
            if j0 + f not in keep:
                g[:, f] = 0


@pytest.mark.parametrize("name", GPU_PLANS)
def test_both_adjoints_are_at_fp32_rounding_of_float64_autograd(name):
    """forward_adjoint with the cotangent in the DC band, band 1 and the last band (every term passes through the fold), and
    backward_adjoint of a random waveform cotangent judged per block, BC = 3, S = 3, against float64 autograd through ref64."""
    base, enc, dec = _fb(name)
    eng, plan = base.nsgt, make_plan(name)
    n, BC = n_for(plan, 3), 3
    G = random_cotangents(plan, BC, 3, seed=BC * 1000 + n % 997)
    _edge_bands_only(plan, G)
    ref = autograd_forward_adjoint(plan, G, n)
    G32 = [g.float() for g in G]
    cpu = forward_adjoint_closed_form(plan, G32, n, dtype=F32)
    got = eng.forward_adjoint(torch.cat([b.reshape(-1) for b in G32]).cuda(), (BC,), n)
    assert got.shape == (BC, n) and bool(torch.isfinite(got).all())
    bad, _ = _judge("fwd_adjoint", f"{name} BC {BC} edge bands", ref64.rel_err(got.cpu(), ref, keep=(0,)), ref64.rel_err(cpu, ref, keep=(0,)),
                    [f"row {r}" for r in range(BC)])
    gy, ref, S = autograd_adjoint(plan, BC, n, seed=BC * 1000 + n % 997)
    gy32 = gy.float()
    cpu = adjoint_closed_form(plan, adjoint_window(plan), gy32, S, dtype=F32)
    got = [v.cpu() for v in eng.table.views(eng.backward_adjoint(gy32.cuda(), S), (BC,), S)]
    b2, _ = _judge("adjoint", f"{name} BC {BC}", _pair([ref64.rel_err(a, r) for a, r in zip(got, ref)]), _pair([ref64.rel_err(c, r) for c, r in zip(cpu, ref)]),
                   _block_labels(plan), full_table=True)
    assert not bad + b2, "\n".join(bad + b2)


# ---- CDAE: every block, both models, pointwise ---------------------------------------------------------------------------------------
CDAE_CASES = [("W", 3, False), ("W", 3, True), ("M", 3, False), ("M", 3, True), ("W", 66, False), ("W", 65, True)]


@pytest.mark.parametrize("name,S,causal", CDAE_CASES)
def test_cdae_masks_of_every_block_are_at_fp32_rounding_of_float64(name, S, causal):
    """ref64 is fed the GPU's own fp32 coefficients, B = 2.  S = 3, and on W S = 66 offline / S = 65 causal: layer-2 / 3 rows of 131 /
    128 positions, so the slab kernels (Winograd F(2, 4)) run on the five- and three-tap blocks, asserted by the profile counters;
    there E is taken over LONG_E_BLOCKS.  All CDAE_ARMS under one cap; bf16x3 must FAIL it.  Arm 3 differs from the default by the
    layer-4 bit alone, which l4f_fits turns off on W: there the two must be BITWISE equal, and on M (offline) they must differ."""
    from xumx_slicq_amd import _lib
    plan, sd = make_plan(name), make_sd(name)
    sep = _sep(name, "realtime" if causal else "offline_phasemix")
    m = sep.xumx_model
    X = sep.nsgt(audio(n_for(plan, S), 2).cuda())
    Xc = [b.cpu() for b in X]
    nb = len(plan.blocks)
    ref = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)]
    e_blocks = list(range(nb)) if S == 3 else LONG_E_BLOCKS
    with one_thread():
        e = _mask_errors([omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(Xc[b]), causal) for b in e_blocks], [ref[b] for b in e_blocks])
    e_cpu = tuple(np.zeros(nb) for _ in range(2))                 # (blocks outside e_blocks carry 0: E is the largest)
    for a, v in zip(e_cpu, e):
        a[e_blocks] = v
    labels = _block_labels(plan)
    bad, kernels = [], {}

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
        kernels[f"{precision} winograd={'default' if wino is None else wino}"] = {k: int(c) for k, (_, c) in sorted(prof.items())}
        return masks

    default, bitwise = None, []
    for precision, wino in CDAE_ARMS:
        masks = run(precision, wino)
        case = f"{name} S={S} causal={causal} {precision} winograd={'default' if wino is None else wino}"
        if default is None:
            default = masks
        elif all(torch.equal(a, b) for a, b in zip(masks, default)):
            bitwise.append(f"{precision} winograd={wino}")
        b, _ = _judge("cdae", case, _mask_errors(masks, ref), e_cpu, labels, full_table=(wino is None and precision == "fp32"))
        if b:
            worst = sorted(range(nb), key=lambda i: -float((masks[i].double() - ref[i]).abs().max()))[:3]
            bad += [f"{case} {msg}" for msg in b] + _logit_report(masks, ref, worst)
    g = _mask_errors(run("bf16x3", None), ref)
    E_rms, E_max = float(e_cpu[0].max()), float(e_cpu[1].max())
    ratio3 = float(np.maximum(g[0] / E_rms, g[1] / E_max).max())
    case = f"{name} S={S} causal={causal}"
    print(f"[cdae] {case} bf16x3: worst e_gpu / E = {ratio3:.1f} (fp32 bound: {M['cdae']}); bitwise the default: {bitwise}")
    print(f"[cdae] {case} kernels of the default: {kernels['fp32 winograd=default']}")
    _TABLES.setdefault("cdae_bf16x3", {})[case] = {"M_key": "cdae/bf16x3 (measured; must exceed M of cdae)", "worst_ratio": ratio3, "E_rms": E_rms, "E_max": E_max}
    _TABLES.setdefault("cdae_kernels", {})[case] = {"M_key": "cdae_kernels (names and launch counts per arm; not judged)", "worst_ratio": 0.0, "arms": kernels,
                                                    "bitwise_the_default": bitwise}
    assert not bad, "\n".join(bad)
    assert ratio3 > M["cdae"], f"bf16x3 passes the fp32 bound ({ratio3:.1f} <= {M['cdae']}): the test cannot see a tenfold loss"
    if S > 3:
        assert {"cdae_l2_slab", "cdae_l3_slab"} <= set(kernels["fp32 winograd=default"]), kernels["fp32 winograd=default"]
    if not causal:
        shapes = FACTS[name][7]
        assert l4f_fits(shapes) == (name != "W")
        assert ("fp32 winograd=3" in bitwise) == (not l4f_fits(shapes)), (name, bitwise)


# ---- Wiener-EM: every block -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("W", 66), ("M", 3)])
def test_wiener_em_of_every_block_is_at_fp32_rounding_of_float64(name, S):
    """W at S = 66, B = 2 with batch row 1 forty times louder (the window maximum is shared over the batch): one to five 5000-frame
    windows per block, the one-band T = 376 block among them; M at S = 3.  The masked form the separator runs (Unmix.forward)
    and the module-level ``blockwise_wiener`` on the same initial magnitudes, both against ref64.blockwise_wiener."""
    from xumx_slicq_amd.phase import blockwise_wiener
    plan = make_plan(name)
    sep = _sep(name, "offline_wiener")
    x = audio(n_for(plan, S), 2)
    x[1] *= 40.0
    X = sep.nsgt(x.cuda())
    Y, masks = sep.xumx_model(X, return_masks=True)
    g_masked, g_module, c = [], [], []
    for b in range(len(plan.blocks)):
        Xb, mb = X[b].cpu(), masks[b].cpu()
        ref = ref64.blockwise_wiener(Xb, mb.double() * ref64.abs_of_real_complex(Xb))
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        ref_m = ref64.blockwise_wiener(Xb, Ymag)
        c.append(ref64.rel_err(omodel.blockwise_wiener(Xb, Ymag), ref_m))
        g_masked.append(ref64.rel_err(Y[b], ref))
        g_module.append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda()), ref_m))
    bad = []
    for tag, g in (("masked (Unmix.forward)", g_masked), ("blockwise_wiener", g_module)):
        b, _ = _judge("wiener", f"{name} S={S} B=2 {tag}", _pair(g), _pair(c), _block_labels(plan, S), full_table=True)
        bad += [f"{tag} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,chunk", [("W", None, 2621440), ("M", None, 2621440), ("M", 40000, 16384)])
@pytest.mark.parametrize("model,causal,wiener", STEM_MODELS)
def test_stems_are_at_fp32_rounding_of_float64(name, n, chunk, model, causal, wiener):
    """Separator.forward against ref64.separate chunk by chunk, per stem, at S = 3 and on M over three chunks (16384 + 16384 + 7232
    samples).  The contractual 1e-4 RMS / 1e-3 max-abs bar is asserted beside the tight one."""
    plan, sd = make_plan(name), make_sd(name)
    n = n_for(plan, 3) if n is None else n
    sep = _sep(name, model)
    x = audio(n, 1)
    keep = sep.chunk_size
    try:
        sep.chunk_size = chunk
        est = sep(x.cuda()).cpu()
    finally:
        sep.chunk_size = keep
    ref = stems_ref(plan, sd, x, causal, wiener, chunk)
    with one_thread():
        orc = osep.separate(plan, sd, x, causal=causal, wiener=wiener, chunk_size=chunk)
    assert est.shape == ref.shape == (4, 1, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (name, model, n, rms, mx)
    bad, _ = _judge("stems", f"{name} {model} n={n}", ref64.rel_err(est, ref, keep=(0,)), ref64.rel_err(orc, ref, keep=(0,)),
                    [f"stem {t}" for t in range(4)], full_table=True)
    assert not bad, "\n".join(bad)


# ---- one training step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_PLANS)
@pytest.mark.parametrize("model", list(TRAIN_MODELS))
def test_training_step_is_at_fp32_rounding_of_float64(name, model):
    """One xsq_train_step at S = 3 (W: B = 1, M: B = 2), offline + Wiener and causal + mix-phase: every gradient tensor and both loss
    terms by the judge of tests/test_ref64_train_gpu.py (its classes, M, RISK, KINK_RTOL and LOOSE_SHARE), then the BatchNorm
    running statistics of a step with the update against ref64.bn_running (its M too)."""
    from xumx_slicq_amd.training import Trainer
    plan, sd = make_plan(name), make_sd(name)
    causal, wiener = TRAIN_MODELS[model]
    sep = _sep(name, "realtime" if causal else "offline_wiener")
    x, y_t = train_inputs(name, plan, train_seed_base(name))
    X, Yt = [c.cpu() for c in sep.nsgt(x.cuda())], [c.cpu() for c in sep.nsgt(y_t.cuda())]
    assert X[0].shape[3] == 3
    r64 = ref64.training_gradients(plan, sd, X, Yt, causal, wiener)
    with one_thread():
        r32 = ref64.training_gradients(plan, sd, X, Yt, causal, wiener, dtype=torch.float32)
    tr = Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), precision="fp32")
    tr.wiener = wiener
    _, mse, msk = tr.step(x, y_t, apply_update=False)
    case = f"plans {name} {model}"
    res = TG._judge_gradients(plan, case, tr.gradients(), mse, msk, r64, r32)
    for stage in ("train/conv", "train/bn", "train/whiten", "train/loss"):
        _T.record(stage, case, TG._T.tables[stage][case])
    TG._assert_case(res)
    tr.step(x, y_t, apply_update=True)
    got = tr.state_dict()
    e_gpu, e_cpu = {}, {}
    for key, (mean, var, count, _, _) in r64[4].items():
        want = ref64.bn_running(sd[key + ".running_mean"], sd[key + ".running_var"], mean, var, count)
        for kind, w, c in zip(("running_mean", "running_var"), want, r32[4][key][3:5]):
            lab = f"layer {key.rsplit('.', 1)[1]} {kind}"
            e_gpu.setdefault(lab, []).append((key, *(float(v) for v in ref64.rel_err(got[f"{key}.{kind}"], w))))
            e_cpu.setdefault(lab, []).append(tuple(float(v) for v in ref64.rel_err(c, w)))
    bad, worst = [], (0.0, "")
    for lab in e_gpu:
        E_rms, E_max = max(e[0] for e in e_cpu[lab]), max(e[1] for e in e_cpu[lab])
        ratios = [(max(r / E_rms, mm / E_max), key) for key, r, mm in e_gpu[lab]]
        worst = max(worst, max(ratios))
        bad += [f"{key} {lab}: {r:.2f} x E" for r, key in ratios if r > TG.M["train/bn_running"]]
    print(f"[train/bn_running] {case}: worst e_gpu / E = {worst[0]:.2f} at {worst[1]}")
    _T.record("train/bn_running", case, {"worst_ratio": worst[0], "worst_at": worst[1]})
    assert not bad, "\n".join(bad[:40])
