"""GPU parity at fp32 rounding on the Mel-32 plan (``fscale = mel, fbins = 32, fmin = 115.5``, L = 2016: the reference's small
streaming models): every band of the sliCQT, every block of the CDAE and of the Wiener-EM filter, and the stems, against the
float64 reference (oracle/ref64.py).  Rule, metric and helper are those of tests/test_ref64_gpu.py:  e_gpu <= M * E  by
``ref64.rel_err``, E the LARGEST fp32-oracle error over the members of the stage on the same input, M per stage a power of two, the
smallest that is at least twice the worst e_gpu / E measured on MI355X, at most ``M_CAP``.  The measured tables are in
profiles/ref64_mel_parity.json, the worst ratio behind every M in DESIGN.md section 2; tests/test_ref64_mel_cpu.py pins the
reference, the plan facts and that no E is zero or noise, and owns the cases both modules use.

What this plan reaches that Bark-262 does not: L is not the length of the hand-written slice FFT, so the default path is the generic
one (slice_window, rocFFT, spectrum_gather with its CSR coverage rows, overlap_add); 33 bands over 1009 bins, the widest a fifth of
the spectrum; nineteen blocks of ONE band; S = 34 slices in a streaming chunk and S = 299 in the long clip.

CDAE arms: the kernel names every arm ran are printed and kept in the tables (stage "cdae_kernels").  The profile counters name
the launch site (cdae_l1_gemm .. cdae_l4_gemm, cdae_l2_slab, cdae_l3_slab), not the variant behind it, so EVERY arm shows the names of
the default on EVERY Mel case, bf16x6 and bf16x3 included; the test therefore also records which arms return the default's masks bit
for bit.  Measured: ``set_winograd(7)`` is the default on all six cases; the offline model's arms 0, 1 and 3 differ from it on every
clip (layers 1 and 4 as F(2, 2) along the hop); the causal model's arms 0, 1, 3 and 7 are ALL bitwise the default at n = 1513 and 32768
-- its layer-2 / 3 rows of 5 .. 68 positions are below the 86 of the slab kernels and F(2, 2) is non-causal only, so these rows are too
short to select an arm -- and on the long clip only arm 0 differs (direct slab kernels instead of Winograd F(2, 4)).

Wall time of the module on MI355X: 13 .. 14 s for its 27 tests (the slowest, the forward transform at n = 1513 with the first rocFFT
plans, 1.4 s).
"""
import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import ref64
from oracle import separator as osep
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables
from test_ref64_gpu import CDAE_ARMS, _forward_inputs, _logit_report, _mask_errors
from test_ref64_mel_cpu import (MASK_LOGIT_SHIFT, MEL, N_CHUNK, N_LONG, N_SHORT, SEED, STEM_CASES, STEM_MODELS, audio, make_mel_plan,
                                make_mel_sd, one_block_inputs, one_thread, residual_share, stems_ref, windows)
from test_wiener_iters_cpu import wiener_iters
from test_wiener_options_cpu import wiener_options

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3             # the contractual bar of tests/test_mel_plan.py, kept beside the tight one

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_mel_parity.json)
M = {
    "forward": 4,                  # 1.52  (n = 1513 impulse, row 1, band 31, Lg 200: rocFFT + radix-4 band kernel)
    "forward/dense_bands": 16,     # 5.36  (n = 1513 synth, band 32, Lg 212: the dense DFT-matrix GEMM sums Lg terms per output in one chain)
    "inverse": 4,                  # 1.12  (n = 1513, all blocks, 7-D, stem 1)
    "inverse/dense_bands": 8,      # 2.13  (n = 32768, block 22 alone, T 212)
    "cdae": 4,                     # 1.56  fp32 (offline, long clip, winograd = 0, block 0), 1.45 bf16x6; bf16x3: 28 .. 41, must fail
    "wiener": 2,                   # 0.69  (blockwise_wiener, block 17, 8 windows)
    "wiener_iters/looped": 2,      # 0.83  (niter = 2, block 0)
    "wiener_iters/resident": 2,    # 0.83  (niter = 2, block 0)
    "wiener_options/masked": 2,    # 0.80  (softmask + residual, niter = 1, block 22, 13 windows)
    "wiener_options/module": 2,    # 0.87  (softmask + residual, niter = 1, block 20, 11 windows)
    "stems": 4,                    # 1.21  (offline mix-phase, n = 500, stem 3)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())

_T = Tables("ref64_mel_parity", M)
_TABLES, _judge = _T.tables, _T.judge
ARMS = ["default", "dense_bands"]          # the default is rocFFT here; short_inline has a test of its own


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


@pytest.fixture(scope="module")
def mel_plan():
    return make_mel_plan()


@pytest.fixture(scope="module")
def mel_sd(mel_plan):
    return make_mel_sd(mel_plan)


@pytest.fixture(scope="module")
def mel_fb():
    from xumx_slicq_amd.transforms import NSGTBase, make_filterbanks
    base = NSGTBase(*MEL, device="cuda")
    enc, dec = make_filterbanks(base)
    return base, enc, dec


@pytest.fixture(scope="module")
def mel_seps():
    from xumx_slicq_amd.separator import seeded_separator
    cfg = dict(fscale=MEL[0], fbins=MEL[1], fmin=MEL[2], seed=SEED)
    seps = {"realtime": seeded_separator(realtime=True, **cfg),
            "offline_phasemix": seeded_separator(realtime=False, wiener=False, **cfg),
            "offline_wiener": seeded_separator(realtime=False, **cfg)}
    yield seps
    for s in seps.values():
        s.drop_graphs()


@pytest.fixture(scope="module")
def mel_sep_shifted():
    """The offline Wiener separator with every last-layer bias lowered by MASK_LOGIT_SHIFT (tests/test_wiener_options_gpu.py)."""
    from xumx_slicq_amd.separator import seeded_separator
    s = seeded_separator(realtime=False, fscale=MEL[0], fbins=MEL[1], fmin=MEL[2], seed=SEED)
    with torch.no_grad():
        for blk in s.xumx_model.sliced_umx:
            for cdae in blk.cdaes:
                cdae[9].bias -= MASK_LOGIT_SHIFT
    s.xumx_model.refresh()
    yield s
    s.drop_graphs()


def _arm(eng, arm):
    return {"default": (lambda: None, lambda: None),
            "dense_bands": (lambda: eng.set_band_radix4(False), lambda: eng.set_band_radix4(True))}[arm]


def _band_labels(plan, rows=None):
    lab = [f"band {j} Lg {int(plan.Lg[j])}" for j in range(plan.nbands)]
    return lab if rows is None else [f"row {r} {l}" for r in rows for l in lab]


def _block_labels(plan, S=None):
    return [f"block {b} F {F} T {T}" + ("" if S is None else f" windows {windows(S, T)[0]}") for b, (_, F, T) in enumerate(plan.blocks)]


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


# ---- forward sliCQT: every band ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_SHORT, N_CHUNK, N_LONG])
def test_forward_every_band_is_at_fp32_rounding_of_float64(mel_fb, mel_plan, n):
    """S = 3, 34 and 299, B = 2; 'synth', 'scaled' (one channel and one batch row at 1e-3, judged per row, channel and band) and
    'impulse' (at the slice seams 2h - 1 and 2h, the last sample and sample 0); the default arm (rocFFT) and every band on the
    dense GEMM; (B, 2, n) and (B, 1, 2, n)."""
    base, enc, dec = mel_fb
    eng, plan = base.nsgt, mel_plan
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
            assert len(C) == 23 and C[0].shape[3] == plan.nslices(n)
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
@pytest.mark.parametrize("n", [N_SHORT, N_CHUNK])
def test_inverse_of_each_block_alone_is_at_fp32_rounding_of_float64(mel_fb, mel_plan, n):
    """Coefficients that are zero except in ONE block, for each of the 23 blocks, stacked along a leading dimension of 23 so one
    call decodes them all (a wrong dual-window value of a band is all of its row's energy); then all blocks at once as the 7-D
    (4, B, 2, ...) input Unmix returns."""
    base, enc, dec = mel_fb
    eng, plan = base.nsgt, mel_plan
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
            b, _ = _judge("inverse", f"n={n} {tag} {arm}", ref64.rel_err(y, ref, keep=(0,)), e_cpu, labels, full_table=(arm == "default"), arm=arm)
            bad += [f"n={n} {tag} {arm} {m}" for m in b]
    assert not bad, "\n".join(bad)


def test_short_inline_is_the_default_path_on_this_plan(mel_fb, mel_plan):
    """The short-band schedule lives in the hand-written slice-FFT kernel, which this plan (L = 2016) cannot run: the switch is
    accepted and changes nothing -- both transforms are bitwise the default's."""
    base, enc, dec = mel_fb
    eng = base.nsgt
    for n in (N_SHORT, N_CHUNK):
        x = audio(n).cuda()
        C = [c.clone() for c in enc(x)]
        y = dec(C, n).clone()
        try:
            eng.set_short_inline(True)
            C1 = [c.clone() for c in enc(x)]
            y1 = dec(C, n).clone()
        finally:
            eng.set_short_inline(False)
        assert all(torch.equal(a, b) for a, b in zip(C, C1)) and torch.equal(y, y1)


# ---- CDAE: all 23 blocks, both models, pointwise ----------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(N_SHORT, 2), (N_CHUNK, 2), (N_LONG, 1)])
@pytest.mark.parametrize("name,causal", [("offline_phasemix", False), ("realtime", True)])
def test_cdae_masks_of_every_block_are_at_fp32_rounding_of_float64(mel_seps, mel_plan, mel_sd, name, causal, n, B):
    """ref64 is fed the GPU's own fp32 coefficients, so only the model is under test.  Rows of S * T positions: 48 .. 636 (S = 3),
    544 .. 7208 (S = 34) and 4784 .. 63388 (S = 299), nineteen blocks of one band; the arms xsq_model_set_winograd 0, 1, 3, 7 and the
    default, and the bf16x6 mode under the same cap.  bf16x3 is measured on the same table and must FAIL the fp32 bound."""
    from xumx_slicq_amd import _lib
    sep = mel_seps[name]
    m = sep.xumx_model
    X = sep.nsgt(audio(n, B).cuda())
    Xc = [b.cpu() for b in X]
    ref = [ref64.cdae_masks(mel_sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)]
    with one_thread():
        e_cpu = _mask_errors([omodel.cdae_masks(mel_sd, b, omodel.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)], ref)
    labels = _block_labels(mel_plan)
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
        print(f"[cdae] {name} n={n} {precision} winograd={wino}: kernels " + ", ".join(f"{k} x{c}" for k, (_, c) in sorted(prof.items())))
        return masks

    default, bitwise = None, []
    for precision, wino in CDAE_ARMS:
        masks = run(precision, wino)
        case = f"{name} n={n} B={B} {precision} winograd={'default' if wino is None else wino}"
        if default is None:
            default = masks
        elif all(torch.equal(a, b) for a, b in zip(masks, default)):
            bitwise.append(f"{precision} winograd={wino}")
        b, _ = _judge("cdae", case, _mask_errors(masks, ref), e_cpu, labels, full_table=(wino is None))
        if b:
            worst = sorted(range(23), key=lambda i: -float((masks[i].double() - ref[i]).abs().max()))[:3]
            bad += [f"{case} {msg}" for msg in b] + _logit_report(masks, ref, worst)
    masks = run("bf16x3", None)
    g = _mask_errors(masks, ref)
    E_rms, E_max = float(e_cpu[0].max()), float(e_cpu[1].max())
    ratio3 = float(np.maximum(g[0] / E_rms, g[1] / E_max).max())
    print(f"[cdae] {name} n={n} bf16x3: worst e_gpu / E = {ratio3:.1f} (fp32 bound: {M['cdae']})")
    _TABLES.setdefault("cdae_bf16x3", {})[f"{name} n={n} B={B}"] = {"M_key": "cdae/bf16x3 (measured; must exceed M of cdae)", "worst_ratio": ratio3, "E_rms": E_rms, "E_max": E_max}
    same = [a for a, k in kernels.items() if a != "fp32 winograd=default" and k == kernels["fp32 winograd=default"]]
    print(f"[cdae] {name} n={n}: arms whose profile names are the default's: {same}")
    print(f"[cdae] {name} n={n}: arms whose masks are bitwise the default's: {bitwise}")
    _TABLES.setdefault("cdae_kernels", {})[f"{name} n={n} B={B}"] = {"M_key": "cdae_kernels (names and launch counts per arm; not judged)", "worst_ratio": 0.0,
                                                                      "arms": kernels, "same_names_as_default": same, "bitwise_the_default": bitwise}
    assert not bad, "\n".join(bad)
    assert ratio3 > M["cdae"], f"bf16x3 passes the fp32 bound ({ratio3:.1f} <= {M['cdae']}): the test cannot see a tenfold loss"


# ---- Wiener-EM: every block -------------------------------------------------------------------------------------------
def _em_inputs(sep):
    """The long clip, B = 2, batch row 1 forty times louder (S = 299): coefficients, estimates and masks of every block."""
    X = sep.nsgt(audio(N_LONG, 2, loud_row=True).cuda())
    Y, masks = sep.xumx_model(X, return_masks=True)
    assert X[0].shape[3] == 299
    return X, Y, masks


@pytest.fixture(scope="module")
def em_inputs(mel_seps):
    return _em_inputs(mel_seps["offline_wiener"])


def test_wiener_em_of_every_block_is_at_fp32_rounding_of_float64(mel_plan, em_inputs):
    """22 of the 23 blocks have one to twelve full 5000-frame windows and a tail; the window maximum is shared over the batch, whose
    row 1 is 40 times louder.  (a) the masked form the separator runs (Unmix.forward) and (b) the module-level ``blockwise_wiener``
    on the same initial magnitudes, both against ref64.blockwise_wiener."""
    from xumx_slicq_amd.phase import blockwise_wiener
    X, Y, masks = em_inputs
    g_masked, g_module, c = [], [], []
    for b in range(23):
        Xb, mb = X[b].cpu(), masks[b].cpu()
        ref = ref64.blockwise_wiener(Xb, mb.double() * ref64.abs_of_real_complex(Xb))
        Ymag = mb * omodel.abs_of_real_complex(Xb)                        # fp32, what the oracle and the module call start from
        ref_m = ref64.blockwise_wiener(Xb, Ymag)
        c.append(ref64.rel_err(omodel.blockwise_wiener(Xb, Ymag), ref_m))
        g_masked.append(ref64.rel_err(Y[b], ref))
        g_module.append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda()), ref_m))
    bad = []
    for tag, g in (("masked (Unmix.forward)", g_masked), ("blockwise_wiener", g_module)):
        b, _ = _judge("wiener", f"n={N_LONG} B=2 {tag}", _pair(g), _pair(c), _block_labels(mel_plan, 299), full_table=True)
        bad += [f"{tag} {m}" for m in b]
    assert not bad, "\n".join(bad)


def test_two_iterations_of_every_block_are_at_fp32_rounding_of_float64(mel_plan, em_inputs):
    """``niter = 2`` on the looped and the window-resident method against the float64 two-iteration helper
    (tests/test_wiener_iters_cpu.py), E from the same loop in complex64."""
    from xumx_slicq_amd.phase import blockwise_wiener
    X, _, masks = em_inputs
    g = {"looped": [], "resident": []}
    c = []
    for b in range(23):
        Xb = X[b].cpu()
        Ymag = masks[b].cpu() * omodel.abs_of_real_complex(Xb)
        ref = wiener_iters(Xb, Ymag, 2)
        c.append(ref64.rel_err(wiener_iters(Xb, Ymag, 2, dtype=torch.complex64), ref))
        for method in g:
            g[method].append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), niter=2, method=method), ref))
    bad = []
    for method, e in g.items():
        b_, _ = _judge("wiener_iters", f"n={N_LONG} B=2 niter=2 {method}", _pair(e), _pair(c), _block_labels(mel_plan, 299), full_table=True, arm=method)
        bad += [f"{method} {m}" for m in b_]
    assert not bad, "\n".join(bad)


def test_softmask_and_residual_of_every_block_are_at_fp32_rounding_of_float64(mel_plan, mel_sep_shifted):
    """``softmask + residual`` at one iteration, five sources, against the float64 helper of tests/test_wiener_options_cpu.py: the
    masked form (Unmix.forward) and the module-level call, on the model with lowered last-layer biases (the share of points with a
    positive residual is asserted)."""
    from xumx_slicq_amd.phase import blockwise_wiener
    sep = mel_sep_shifted
    X, _, masks = _em_inputs(sep)
    try:
        sep.softmask, sep.residual = True, True
        Y = sep.xumx_model(X)
    finally:
        sep.softmask, sep.residual = False, False
    share = residual_share([(X[b].cpu(), masks[b].cpu()) for b in range(23)])
    print(f"share of points with a positive residual: {share:.3f} (mask logit shift {MASK_LOGIT_SHIFT})")
    assert 0.1 <= share <= 0.9, share
    g = {"masked": [], "module": []}
    c = []
    for b in range(23):
        Xb, mb = X[b].cpu(), masks[b].cpu()
        assert Y[b].shape == (5, *Xb.shape)
        ref = wiener_options(Xb, mb.double() * ref64.abs_of_real_complex(Xb), 1, True, True)
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        ref_m = wiener_options(Xb, Ymag, 1, True, True)
        c.append(ref64.rel_err(wiener_options(Xb, Ymag, 1, True, True, dtype=torch.complex64), ref_m))
        g["masked"].append(ref64.rel_err(Y[b], ref))
        g["module"].append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), niter=1, softmask=True, residual=True), ref_m))
    bad = []
    for arm, e in g.items():
        b_, _ = _judge("wiener_options", f"n={N_LONG} B=2 softmask=1 residual=1 niter=1 {arm}", _pair(e), _pair(c), _block_labels(mel_plan, 299),
                       full_table=True, arm=arm)
        bad += [f"{arm} {m}" for m in b_]
    assert not bad, "\n".join(bad)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk", STEM_CASES)
@pytest.mark.parametrize("name,causal,wiener", STEM_MODELS)
def test_stems_are_at_fp32_rounding_of_float64(mel_seps, mel_plan, mel_sd, name, causal, wiener, n, chunk):
    """Separator.forward against ref64.separate chunk by chunk, per stem: a clip shorter than a slice (n = 500, padded to L / 2 + 1
    samples), S = 3, a full streaming chunk of 32,768 samples followed by a tail of 7232, and the long clip in one chunk.  The
    contractual 1e-4 RMS / 1e-3 max-abs bar is asserted beside the tight one."""
    sep = mel_seps[name]
    x = audio(n, 1)
    keep = sep.chunk_size
    try:
        sep.chunk_size = chunk
        est = sep(x.cuda()).cpu()
    finally:
        sep.chunk_size = keep
    ref = stems_ref(mel_plan, mel_sd, x, causal, wiener, chunk)
    with one_thread():
        orc = osep.separate(mel_plan, mel_sd, x, causal=causal, wiener=wiener, chunk_size=chunk)
    assert est.shape == ref.shape == (4, 1, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (name, n, rms, mx)
    bad, _ = _judge("stems", f"{name} n={n}", ref64.rel_err(est, ref, keep=(0,)), ref64.rel_err(orc, ref, keep=(0,)),
                    [f"stem {t}" for t in range(4)], full_table=True)
    assert not bad, "\n".join(bad)
