"""Plans with bands across DC on the device (``dc_twins=True``): the mirrored synthesis of the reference's inverse (k_twin_synthesis,
csrc/dc_twins.h) and its transpose (k_twin_analysis), and everything that runs on such a plan for the first time -- the forward
transform and its adjoint, the F = 10 three-tap and F = 20 five-tap first blocks of the CDAE, the separator's entry points and the
ideal-mask oracle.  The CPU facts are in tests/test_dc_twins_cpu.py and tests/test_ref64_plans_cpu.py, which owns the plans:

  T = ``bark, 28, 32.9`` (L 1872) and K = ``bark, 56, 32.9`` (L 3808): band 1 (c 2, q = 2..7 -> bins 0..5) and band 2 (c 6, q = 6, 7 ->
  bins 0, 1): 8 landing entries, two bands meeting on bins 0 and 1.  Mel-32 (one band, share 0.0084): dropped by default, computed
  with the flag.  Bark-262: no such band; the flag changes no bit.

Rule, metric and helpers are those of tests/test_ref64_plans_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err``, E the fp32 CPU oracle's
error against float64 on the same input, M per stage the smallest power of two at least twice the worst ratio measured on MI355X
(profiles/dc_twins_parity.json), at most ``M_CAP``.  Shapes: n = n_for(plan, 3) (1795 / 3731 samples, S = 3: even and odd slices in
one call), B = 2 or BC = 3 (row parity and slice parity disagree).

Wall time of the module on MI355X: 14 s for its 26 tests in one process (the slowest, the evaluator and its three-round search, 4.0 s;
every other test 1.3 s or less).
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
from test_autograd_cpu import F32, F64, autograd_forward_adjoint, forward_adjoint_closed_form, random_cotangents
from test_dc_twins_cpu import twin_adjoint_closed_form
from test_ref64_gpu import CDAE_ARMS, _mask_errors
from test_ref64_mel_cpu import one_block_inputs, one_thread, stems_ref
from test_ref64_plans_cpu import PLANS, SEED, STEM_MODELS, audio, make_plan, make_sd, n_for
from test_remix_gpu import _close_to_einsum
from test_sdr_cpu import adjoint_closed_form, adjoint_window, autograd_adjoint

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3             # the contractual bar
CFG = {"T": PLANS["T"], "K": PLANS["K"], "mel32": ("mel", 32, 115.5), "bark262": ("bark", 262, 32.9)}

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/dc_twins_parity.json)
M = {
    "inverse": 4,                  # 1.07  (K, all blocks 7-D, stem 3); Mel-32 with the flag 1.03
    "inverse/dense_bands": 8,      # 2.30  (K, block 31 alone, T 272: the dense GEMM sums 2 Lg terms per output in one chain)
    "inverse_masked": 4,           # 1.19  (T, BC 8 over BCx 2, row 7)
    "fwd_adjoint": 4,              # 1.06  (T, BC 3, cotangent in bands 0, 1, 2 and 28: row 1)
    "adjoint": 4,                  # 1.45  (K, BC 3: block 0, F 20, T 16 -- the block of both bands across DC)
    "roundtrip_grad": 4,           # 1.03  (T, B 2, row 0)
    "cdae": 4,                     # 1.93  (K offline, bf16x6: block 0, F 20, T 16); fp32 arms at most 1.50
    "stems": 4,                    # 1.19  (K, realtime, stem 0)
}
# without the mirrored synthesis float64 itself is 2.3e5 x E on block 0 of T (asserted to exceed M of "inverse")
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("dc_twins_parity", M)
_judge = _T.judge
ARMS = ["default", "dense_bands"]


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


_FB, _SEPS = {}, {}


def _plan(name):
    return make_plan(name) if name in PLANS else O.make_plan(*CFG[name])


def _fb(name, dc_twins=True):
    if (name, dc_twins) not in _FB:
        from xumx_slicq_amd.transforms import NSGTBase, make_filterbanks
        base = NSGTBase(*CFG[name], device="cuda", dc_twins=dc_twins)
        _FB[name, dc_twins] = (base, *make_filterbanks(base))
    return _FB[name, dc_twins]


def _sep(name, model):
    if (name, model) not in _SEPS:
        from xumx_slicq_amd.separator import seeded_separator
        cfg = dict(fscale=CFG[name][0], fbins=CFG[name][1], fmin=CFG[name][2], seed=SEED, dc_twins=True)
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


def _block_labels(plan):
    return [f"block {b} F {F} T {T}" for b, (_, F, T) in enumerate(plan.blocks)]


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


def _ratio(e, e_cpu, i=0):
    """e / E of member i, by the judge's formula (E = the largest e_cpu per metric)."""
    return max(float(np.asarray(e[0]).reshape(-1)[i]) / float(np.max(e_cpu[0])), float(np.asarray(e[1]).reshape(-1)[i]) / float(np.max(e_cpu[1])))


def _num_twins(eng):
    from xumx_slicq_amd import _lib
    return int(_lib.lib.xsq_plan_num_twins(eng.handle(torch.device("cuda", torch.cuda.current_device()))))


# ---- 1. the inverse, block by block ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T", "K"])
def test_inverse_of_each_block_alone_is_at_fp32_rounding_of_float64(name):
    """Coefficients that are zero except in ONE block, for each block, stacked along a leading dimension (row (k, ch), S = 3: row
    parity and slice parity disagree); then all blocks as the 7-D (4, B, 2, ...) input.  Against ``ref64.inverse``, which on these
    plans synthesises the twins by default; the default arm and every band on the dense GEMM.  And the test can see a dropped
    term: ``ref64.inverse(..., twins=False)`` is itself outside M * E on block 0, which holds both bands across DC."""
    base, enc, dec = _fb(name)
    eng, plan = base.nsgt, make_plan(name)
    assert base.plan.dc_twins and _num_twins(eng) == 8
    n = n_for(plan, 3)
    P, Q = one_block_inputs(plan, n)
    bad = []
    for tag, X, labels in (("one block", P, _block_labels(plan)), ("all blocks 7-D", Q, [f"stem {t}" for t in range(4)])):
        ref = ref64.inverse(plan, X, n)
        e_cpu = ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,))
        if tag == "one block":
            dropped = _ratio(ref64.rel_err(ref64.inverse(plan, X, n, twins=False).float(), ref, keep=(0,)), e_cpu, 0)
            print(f"[inverse] {name}: without the mirrored synthesis block 0 is {dropped:.3g} x E")
            _T.record("inverse_without_twins", f"{name} block 0", {"M_key": "inverse_without_twins (float64 without the term, over E; must exceed M of inverse)",
                                                                   "worst_ratio": dropped})
            assert dropped > M["inverse"], (name, dropped)
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


# ---- 2. the reference's own numbers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T", "K"])
def test_transforms_equal_the_reference_fixture(name):
    """tests/golden/plans3_<name>.npz: forward coefficients at 2e-5, the decode from all blocks and from block 0 alone at 1e-4 RMS /
    1e-3 max-abs (without the term: 5.2e-3 and 1.1e-3 max-abs, tests/test_ref64_plans_cpu.py)."""
    from xumx_slicq_amd.synth import synth_audio
    base, enc, dec = _fb(name)
    g = load_golden(f"plans3_{name}.npz")
    n = int(g["n"])
    C = enc(synth_audio(n, seed=20260101 + n).cuda())
    assert len(C) == len(base.plan.blocks) and all(f"fwd_{i}" in g for i in range(len(C)))
    for i, cb in enumerate(C):
        assert float((cb.cpu() - torch.from_numpy(g[f"fwd_{i}"])).abs().max()) < 2e-5, (name, i)
    for key, X in (("inv", C), ("inv_block0", [c if i == 0 else torch.zeros_like(c) for i, c in enumerate(C)])):
        d = dec(X, n).cpu().double() - torch.from_numpy(g[key]).double()
        rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
        print(f"[fixture] {name} {key}: GPU decode against the reference's: rms {rms:.2e} max {mx:.2e}")
        _T.record("fixture", f"{name} {key}", {"M_key": "fixture (absolute distance from the reference's decode; bar 1e-4 RMS / 1e-3 max)", "worst_ratio": mx / MAX_TOL,
                                               "rms": rms, "max": mx})
        assert rms < RMS_TOL and mx < MAX_TOL, (name, key, rms, mx)


# ---- 3. the masked form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T", "K"])
def test_masked_inverse_is_at_fp32_rounding_of_float64(name):
    """``backward_masked`` with BC = 8 mask channels over BCx = 2 mix channels: the inverse of masks[bc] * mix[bc % 2], the product
    rounded to fp32 as the kernels round it, against ``ref64.inverse`` of that product."""
    base, enc, dec = _fb(name)
    eng, plan = base.nsgt, make_plan(name)
    n, BC, BCx, S = n_for(plan, 3), 8, 2, 3
    gen = torch.Generator().manual_seed(n + 8)
    mix = [torch.randn(BCx, F, S, T, 2, generator=gen) for (_, F, T) in plan.blocks]
    masks = [torch.rand(BC, F, S, T, generator=gen) for (_, F, T) in plan.blocks]
    X = [mk[..., None] * mx.repeat(BC // BCx, 1, 1, 1, 1) for mk, mx in zip(masks, mix)]           # row bc reads mix row bc % BCx
    ref = ref64.inverse(plan, X, n)
    e_cpu = ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,))
    out = torch.empty(BC, n, dtype=torch.float32, device="cuda")
    offs = (torch.arange(BC, dtype=torch.int64) * n).cuda()
    eng.backward_masked(torch.cat([m.reshape(-1) for m in masks]).cuda(), torch.cat([m.reshape(-1) for m in mix]).cuda(), BC, BCx, S, n, out, offs)
    bad, _ = _judge("inverse_masked", f"{name} BC {BC} BCx {BCx}", ref64.rel_err(out.cpu(), ref, keep=(0,)), e_cpu, [f"row {r}" for r in range(BC)], full_table=True)
    assert not bad, "\n".join(bad)


# ---- 4. both adjoints ------------------------------------------------------------------------------------------------------------------
def _edge_bands_only(plan, G):
    keep = {0, 1, 2, plan.nbands - 1}
    for (j0, F, T), g in zip(plan.blocks, G):
        for f in range(F):
            if j0 + f not in keep:
                g[:, f] = 0


@pytest.mark.parametrize("name", ["T", "K"])
def test_both_adjoints_are_at_fp32_rounding_of_float64_autograd(name):
    """BC = 3, S = 3, against float64 autograd through ref64.  forward_adjoint (the analysis has no twin: unchanged kernels, first
    run on these plans) with the cotangent in the DC band, bands 1 and 2 and the last band; backward_adjoint of a random waveform
    cotangent per block, and accumulated onto a seeded arena.  E of backward_adjoint: the closed form over a' plus the closed form
    of the twin term (tests/test_dc_twins_cpu.py), both in fp32."""
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
    cpu = [a + t for a, t in zip(adjoint_closed_form(plan, adjoint_window(plan), gy32, S, dtype=F32), twin_adjoint_closed_form(plan, gy32, S, plan.twins, F32))]
    e_cpu = _pair([ref64.rel_err(c, r) for c, r in zip(cpu, ref)])
    arena = eng.backward_adjoint(gy32.cuda(), S)
    got = [v.cpu() for v in eng.table.views(arena, (BC,), S)]
    b2, _ = _judge("adjoint", f"{name} BC {BC}", _pair([ref64.rel_err(a, r) for a, r in zip(got, ref)]), e_cpu, _block_labels(plan), full_table=True)
    # accumulate = 1: the same gradient, twin term included, computed in the workspace and added onto what the arena held by ONE
    # fp32 addition per entry -- bitwise the sum of the seed and the arena above
    seeded = torch.randn(arena.shape, generator=torch.Generator().manual_seed(3)).cuda()
    acc = eng.backward_adjoint(gy32.cuda(), S, out=seeded.clone())
    assert torch.equal(acc, seeded + arena), name
    assert not bad + b2, "\n".join(bad + b2)


def test_gradient_through_the_round_trip_on_t():
    """One ``loss.backward()`` through ``INSGT_SL(NSGT_SL(x))``: d <y, w> / dx against float64 autograd through
    ``ref64.inverse(ref64.forward(x))``; E: the same through the fp32 oracle."""
    base, enc, dec = _fb("T")
    plan = make_plan("T")
    n, B = n_for(plan, 3), 2
    x = audio(n, B)                                                                       # (B, 2, n)
    w = torch.randn(B, 2, n, generator=torch.Generator().manual_seed(n + 3), dtype=F64)
    x64 = x.double().requires_grad_(True)
    (ref64.inverse(plan, ref64.forward(plan, x64), n) * w).sum().backward()
    x32 = x.clone().requires_grad_(True)
    (O.inverse(plan, O.forward(plan, x32), n) * w.float()).sum().backward()
    xd = x.cuda().requires_grad_(True)
    (dec(enc(xd), n) * w.float().cuda()).sum().backward()
    assert xd.grad is not None and xd.grad.shape == (B, 2, n)
    bad, _ = _judge("roundtrip_grad", f"T B {B}", ref64.rel_err(xd.grad.cpu().reshape(2 * B, n), x64.grad.reshape(2 * B, n), keep=(0,)),
                    ref64.rel_err(x32.grad.reshape(2 * B, n), x64.grad.reshape(2 * B, n), keep=(0,)), [f"row {r}" for r in range(2 * B)])
    assert not bad, "\n".join(bad)


# ---- 5. Mel-32 with the term, Bark-262 unmoved -------------------------------------------------------------------------------------------
def test_mel32_with_the_flag_decodes_with_the_term():
    """Against ``ref64.inverse(..., twins=True)``; and the term is visible: the default engine's decode of the same coefficients is
    judged against the same reference and the two differ."""
    base, enc, dec = _fb("mel32")
    plan = _plan("mel32")
    assert _num_twins(base.nsgt) == 2
    n = n_for(plan, 3)
    P, _ = one_block_inputs(plan, n)
    ref = ref64.inverse(plan, P, n, twins=True)
    e_cpu = ref64.rel_err(O.inverse(plan, P, n, twins=True), ref, keep=(0,))
    Xd = [p.cuda() for p in P]
    y = dec(Xd, n).cpu()
    bad, _ = _judge("inverse", "mel32 one block", ref64.rel_err(y, ref, keep=(0,)), e_cpu, _block_labels(plan), full_table=True)
    assert not bad, "\n".join(bad)
    _, _, dec0 = _fb("mel32", dc_twins=False)
    assert _num_twins(_fb("mel32", dc_twins=False)[0].nsgt) == 0
    y0 = dec0(Xd, n).cpu()
    assert plan.blocks[0] == (0, 9, 16) and [t[0] for t in plan.twins] == [1]             # the band across DC lies in block 0
    assert not torch.equal(y0[0], y[0]) and torch.equal(y0[1:], y[1:])                   # the other blocks alone: no bit moves
    e0 = ref64.rel_err(y0, ref, keep=(0,))
    assert int(np.argmax(e0[0])) == 0 and _ratio(e0, e_cpu, 0) > M["inverse"], (e0[0][:3], e_cpu[0][:3])


def test_bark262_with_the_flag_is_bitwise_the_default_engine():
    base, enc, dec = _fb("bark262")
    base0, enc0, dec0 = _fb("bark262", dc_twins=False)
    assert base.plan.dc_twins and base.plan.twins == [] and _num_twins(base.nsgt) == 0 == _num_twins(base0.nsgt)
    x = audio(9031, 2).cuda()
    C, C0 = enc(x), enc0(x)
    assert all(torch.equal(a, b) for a, b in zip(C, C0))
    assert torch.equal(dec(C, 9031), dec0(C0, 9031))


# ---- 6. the CDAE on its F = 10 and F = 20 first blocks, and the stems -----------------------------------------------------------------
@pytest.mark.parametrize("name,causal", [("T", False), ("T", True), ("K", False), ("K", True)])
def test_cdae_masks_of_every_block_are_at_fp32_rounding_of_float64(name, causal):
    """ref64 is fed the GPU's own fp32 coefficients, B = 2, S = 3; every arm of CDAE_ARMS under one cap.  The first GPU run of the
    F = 10 three-tap (T) and F = 20 five-tap (K) first blocks."""
    plan, sd = make_plan(name), make_sd(name)
    sep = _sep(name, "realtime" if causal else "offline_phasemix")
    m = sep.xumx_model
    X = sep.nsgt(audio(n_for(plan, 3), 2).cuda())
    Xc = [b.cpu() for b in X]
    assert Xc[0].shape[2:4] == (plan.blocks[0][1], 3) and plan.blocks[0][1] == {"T": 10, "K": 20}[name]
    ref = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)]
    with one_thread():
        e_cpu = _mask_errors([omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(Xb), causal) for b, Xb in enumerate(Xc)], ref)
    bad = []
    for precision, wino in CDAE_ARMS:
        try:
            m.set_precision(precision)
            if wino is not None:
                m.set_winograd(wino)
            _, masks = m(X, return_masks=True)
            masks = [k.cpu() for k in masks]
        finally:
            m.set_precision("fp32")
            m.set_winograd(True)
        case = f"{name} S=3 causal={causal} {precision} winograd={'default' if wino is None else wino}"
        b, _ = _judge("cdae", case, _mask_errors(masks, ref), e_cpu, _block_labels(plan), full_table=(wino is None and precision == "fp32"))
        bad += [f"{case} {msg}" for msg in b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["T", "K"])
@pytest.mark.parametrize("model,causal,wiener", STEM_MODELS)
def test_stems_are_at_fp32_rounding_of_float64(name, model, causal, wiener):
    """Separator.forward against ref64.separate (twins live on these plans), per stem, at the contractual bar and at the judge's."""
    plan, sd = make_plan(name), make_sd(name)
    n = n_for(plan, 3)
    sep = _sep(name, model)
    assert sep.dc_twins
    x = audio(n, 1)
    est = sep(x.cuda()).cpu()
    ref = stems_ref(plan, sd, x, causal, wiener, 2621440)
    with one_thread():
        orc = osep.separate(plan, sd, x, causal=causal, wiener=wiener, chunk_size=2621440)
    assert est.shape == ref.shape == (4, 1, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (name, model, n, rms, mx)
    bad, _ = _judge("stems", f"{name} {model} n={n}", ref64.rel_err(est, ref, keep=(0,)), ref64.rel_err(orc, ref, keep=(0,)),
                    [f"stem {t}" for t in range(4)], full_table=True)
    assert not bad, "\n".join(bad)


# ---- 7. the other entry points of the separator, on T -----------------------------------------------------------------------------------
def test_graphed_forward_is_bitwise_forward_and_remix_is_the_weighted_sum_on_t():
    plan = make_plan("T")
    sep = _sep("T", "offline_phasemix")
    x = audio(n_for(plan, 3), 2).cuda()
    stems = sep(x)
    assert torch.equal(sep.forward_graphed(x), stems)
    assert torch.equal(sep.forward_graphed(x), stems)                                    # the replay
    karaoke = [[1.0, 0.0, 1.0, 1.0]]                                                     # everything but the vocals
    got = sep.remix(x, torch.tensor(karaoke))
    assert got.shape == (1, 2, 2, x.shape[-1])
    _close_to_einsum(got, stems, karaoke)
    # cross-faded segments (883 samples per hop, 88 shared): the one native call against its definition, at the contractual bar
    from xumx_slicq_amd.separator import overlapped_loop
    seg = sep.forward_overlapped(x, segment=0.02, overlap=0.002)
    chunk_len, ov = sep._segment_lengths(0.02, 0.002)
    d = (seg - overlapped_loop(sep.forward, x, chunk_len, ov)).double()
    assert seg.shape == stems.shape and float(d.pow(2).mean().sqrt()) < RMS_TOL and float(d.abs().max()) < MAX_TOL


# ---- 8. the ideal-mask oracle and the parameter search ------------------------------------------------------------------------------------
def _dc_fixture_tool():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("make_golden_ideal_dc", os.path.join(ROOT, "tools", "make_golden_ideal_dc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("key", ["t4w", "t4p"])
def test_ideal_oracle_equals_the_reference_fixture_on_t(key):
    """tests/golden/ideal_oracle_dc.npz (tools/make_golden_ideal_dc.py: the reference's ``ideal_slicqt`` on T, n = 4001, one stereo
    item): estimates at 1e-4 RMS / 1e-3 max-abs, SDRs within 1e-3 dB -- the bars of tests/test_slicqfinder_gpu.py."""
    from xumx_slicq_amd import scoring
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    G = _dc_fixture_tool()
    g = load_golden("ideal_oracle_dc.npz")
    assert G.PLAN == PLANS["T"] and G.CASES[key][0] == 4001
    src = torch.from_numpy(G.case_sources(key))[:, None].contiguous().cuda()               # (4, 1, 2, n)
    est = ideal_slicqt(src, _fb("T")[0], G.CASES[key][1])
    ref = torch.from_numpy(np.stack([g[f"est_{key}_{j}"] for j in range(4)]))[:, None]
    d = est.cpu() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    res = scoring.score(est, src, target_order=G.SOURCES, estimate_order=G.SOURCES)["targets"]
    sdr = np.asarray([res[t]["sdr_global"][0] for t in G.SOURCES])
    want = g[f"sdr_{key}"]
    print(f"\n{key}: rms {rms:.3e} max {mx:.3e}; sdr diff {np.abs(sdr - want).max():.3e} dB")
    _T.record("fixture", f"ideal {key}", {"M_key": "fixture (absolute distance from the reference's decode; bar 1e-4 RMS / 1e-3 max)", "worst_ratio": mx / MAX_TOL,
                                          "rms": rms, "max": mx, "sdr_diff_db": float(np.abs(sdr - want).max())})
    assert bool(torch.isfinite(est).all())
    assert rms < 1e-4 and mx < 1e-3, (rms, mx)
    assert np.abs(sdr - want).max() < 1e-3, (sdr, want)


def test_track_evaluator_and_search_score_plans_across_dc():
    from test_slicqfinder_gpu import tiny_dataset
    from xumx_slicq_amd.slicqfinder import TrackEvaluator, optimize_many
    ev = TrackEvaluator(tiny_dataset(), dc_twins=True)
    got = ev.oracle("bark", 32.9, 28)
    assert len(got) == 4 and all(np.isfinite(got)) and ev.refusals == []
    assert TrackEvaluator(tiny_dataset()).oracle("bark", 32.9, 28) == (float("-inf"),) * 4        # the default still refuses
    ev1 = TrackEvaluator(tiny_dataset(), tracks=[1], dc_twins=True)
    # (the ranges of tests/test_slicqfinder_gpu.py, which reach plans with a band across DC: there several draws are refused)
    res = optimize_many(ev1.oracle, {"scales": ["bark", "mel"], "bins": (24, 40), "fmin": (30.0, 130.0, 0.5)}, 3, seed=7, refusals=ev1.refusals,
                        dc_twins=ev1.dc_twins)
    assert len(res["rounds"]) == 3 and res["dc_twins"] is True
    assert not any("plan refused" in r["reason"] for r in res["refusals"]) and res["rerolled"] == 0 and ev1.refusals == []


# ---- 9. what stays refused -------------------------------------------------------------------------------------------------------------
def test_stream_trainer_and_sharding_refuse_naming_dc_twins():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.training import Trainer
    sep = _sep("T", "realtime")
    with pytest.raises(_lib.XsqError, match="dc_twins"):
        sep.stream()
    with pytest.raises(_lib.XsqError, match="dc_twins"):
        Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), precision="fp32")
    n = n_for(make_plan("T"), 3)
    with pytest.raises(_lib.XsqError, match="dc_twins"):
        sep.demix_into(audio(n, 1).cuda(), torch.empty(4, 1, 2, n, device="cuda"), torch.zeros(4, 1, 2, dtype=torch.int64, device="cuda"))
    assert _num_twins(_fb("T")[0].nsgt) == 8
    from xumx_slicq_amd.transforms import NSGTBase
    w = NSGTBase(*PLANS["W"], device="cuda")
    assert _num_twins(w.nsgt) == 0
    w.nsgt.close()
