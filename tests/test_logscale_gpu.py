"""The FFT band engine (csrc/band_fft.h) on the device: plans made with ``long_bands=True`` on the logarithmic scales, whose bands
above Lg 320 it runs -- both transforms, both adjoints, the masked inverse, the ideal-mask oracle, the spectrogram and the search.
tests/test_logscale_cpu.py owns the plans (A = ``cqlog, 10, 130.0``, B = ``vqlog, 24, 40.0``, C = ``cqlog, 12, 20.0``; D = ``cqlog,
15, 12.0`` for the 8192-point FFT class), the shapes (n = 2 h + 1: S = 3, and n = 7 h + 123: S = 5 with a ragged tail; BC = 1 and 3)
and the helpers.

Rule, metric and helpers are those of tests/test_ref64_plans_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err``, per band for the forward
transform and per block for the inverse; E the fp32 CPU oracle's error against float64 (oracle/ref64.py) on the same input, both over
an ``oracle.slicqt.Plan`` filled from the package plan's fields; M per stage the smallest power of two at least twice the worst ratio
measured on MI355X (profiles/logscale_parity.json), at most ``M_CAP``.  The float64 comparisons run on the default engine
(``dc_twins=False``: the 0.007 share of A and C is dropped by contract, as ``ref64.inverse`` drops it) and, for the inverse of A, with
the twin; the reference's fixture (tests/golden/logscale*.npz) is met with ``dc_twins=True``.

Wall time of the module on MI355X: 15 s for its 32 tests in one process (the slowest, the inverse and the forward of B with their
float64 references, 1.9 and 1.7 s; the case of D 1.4 s; everything but those seven cases 0.3 s or less).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import ref64
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables
from test_autograd_cpu import F32, F64, autograd_forward_adjoint, forward_adjoint_closed_form, random_cotangents
from test_logscale_cpu import CONFIGS, G, PLANS, audio, lengths, oracle_plan
from test_ref64_mel_cpu import one_block_inputs
from test_sdr_cpu import adjoint_closed_form, adjoint_window, autograd_adjoint
from test_spectrogram_cpu import ref_block_db, ref_block_magnitude, ref_columns

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3             # the contractual bar

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/logscale_parity.json)
M = {
    "forward": 4,                  # 1.70  (A, n 1175, BC 1: band 10, Lg 1020; B and C at most 0.97; D 1.20 at band 12, Lg 3044, and 1.16 / 1.19
                                   #        on its 8192-point bands, Lg 8592 / 11240)
    "inverse": 4,                  # 1.64  (D, one block alone: block 1, T 24; its 8192-point blocks T 8592 / 11240: 1.15 / 1.29; A 1.31, all
                                   #        blocks 7-D, stem 2)
    "inverse_masked": 4,           # 1.47  (A, n 4232, BC 3 over BCx 1, row 1; five (n, BC, BCx) cases per plan)
    "fwd_adjoint": 4,              # 1.27  (A, n 1175, BC 1; four shapes per plan)
    "adjoint": 4,                  # 1.30  (A, n 1175, BC 1: block 7, T 768; four shapes per plan)
    "roundtrip": 4,                # 1.70  (A, the gradient, n 1175, BC 3, row 1; the reconstruction itself 1.53)
    "spectrogram/db": 4,           # 1.49  (C, block 10, T 6416; the M of tests/test_spectrogram_gpu.py)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("logscale_parity", M)
_judge = _T.judge
SHAPES = [(0, 1), (0, 3), (1, 1), (1, 3)]          # (index into lengths(plan), BC)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


_FB = {}


def _fb(key, dc_twins=False):
    if (key, dc_twins) not in _FB:
        from xumx_slicq_amd.transforms import NSGTBase, make_filterbanks
        scale, fbins, fmin, fgamma = CONFIGS[key]
        base = NSGTBase(scale, fbins, fmin, fgamma=fgamma, device="cuda", dc_twins=dc_twins, long_bands=True)
        _FB[key, dc_twins] = (base, *make_filterbanks(base))
    return _FB[key, dc_twins]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for base, _, _ in _FB.values():
        base.nsgt.close()
    _FB.clear()


def _num_long(eng):
    from xumx_slicq_amd import _lib
    return int(_lib.lib.xsq_plan_num_long_bands(eng.handle(torch.device("cuda", torch.cuda.current_device()))))


def _band_labels(plan, rows):
    return [f"row {r} band {j} Lg {int(plan.Lg[j])}" for r in range(rows) for j in range(plan.nbands)]


def _block_labels(plan):
    return [f"block {b} F {F} T {T}" for b, (_, F, T) in enumerate(plan.blocks)]


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


def _random_blocks(plan, BC, S, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(BC, F, S, T, 2, generator=gen) for (_, F, T) in plan.blocks]


# ---- 1. forward: every band -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(PLANS))
def test_forward_every_band_is_at_fp32_rounding_of_float64(key):
    base, enc, dec = _fb(key)
    plan = oracle_plan(key)
    assert _num_long(base.nsgt) == int((plan.Lg > 320).sum()) > 0
    bad = []
    for li, BC in SHAPES:
        n = lengths(plan)[li]
        x = audio(n, BC)
        ref = ref64.forward(plan, x)
        e_cpu = ref64.band_rel_err(O.forward(plan, x), ref, True)
        C = [c.cpu() for c in enc(x.cuda())]
        assert len(C) == len(plan.blocks) and C[0].shape[-3] == (3, 5)[li] and all(bool(torch.isfinite(c).all()) for c in C)
        b, _ = _judge("forward", f"{key} n {n} BC {BC}", tuple(e.reshape(-1) for e in ref64.band_rel_err(C, ref, True)),
                      tuple(e.reshape(-1) for e in e_cpu), _band_labels(plan, BC), full_table=(BC == 3 and li == 0))
        bad += [f"{key} n {n} BC {BC} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- 2. inverse: one block at a time, and random coefficients at every shape ---------------------------------------------------------------
@pytest.mark.parametrize("key", list(PLANS))
def test_inverse_of_each_block_alone_is_at_fp32_rounding_of_float64(key):
    """Coefficients that are zero except in ONE block, for each block, stacked along a leading dimension (S = 3); then all blocks as
    the 7-D (4, B, 2, ...) input; then random coefficients at the four shapes, per row."""
    base, enc, dec = _fb(key)
    plan = oracle_plan(key)
    n = lengths(plan)[0]
    P, Q = one_block_inputs(plan, n)
    bad = []
    for tag, X, labels in (("one block", P, _block_labels(plan)), ("all blocks 7-D", Q, [f"stem {t}" for t in range(4)])):
        ref = ref64.inverse(plan, X, n)
        e_cpu = ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,))
        y = dec([p.cuda() for p in X], n).cpu()
        assert y.shape == ref.shape
        b, _ = _judge("inverse", f"{key} {tag}", ref64.rel_err(y, ref, keep=(0,)), e_cpu, labels, full_table=True)
        bad += [f"{key} {tag} {m}" for m in b]
    for li, BC in SHAPES:
        n = lengths(plan)[li]
        X = _random_blocks(plan, BC, (3, 5)[li], n + BC)
        ref = ref64.inverse(plan, X, n)
        y = dec([p.cuda() for p in X], n).cpu()
        b, _ = _judge("inverse", f"{key} random n {n} BC {BC}", ref64.rel_err(y, ref, keep=(0,)), ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)),
                      [f"row {r}" for r in range(BC)])
        bad += [f"{key} n {n} BC {BC} {m}" for m in b]
    assert not bad, "\n".join(bad)


def test_the_largest_fft_class_is_at_fp32_rounding_of_float64():
    """D = ``cqlog, 15, 12.0``: Lg 8592 and 11240 run through the 8192-point FFT, 64 KB of LDS, the largest the engine launches.
    Forward per band and inverse per block at S = 3, BC = 1, under the M of A, B and C."""
    base, enc, dec = _fb("D")
    plan = oracle_plan("D")
    assert _num_long(base.nsgt) == 8 and int(plan.Lg.max()) == 11240
    n = lengths(plan)[0]
    x = audio(n, 1)
    ref = ref64.forward(plan, x)
    C = [c.cpu() for c in enc(x.cuda())]
    bad, _ = _judge("forward", f"D n {n} BC 1", tuple(e.reshape(-1) for e in ref64.band_rel_err(C, ref, True)),
                    tuple(e.reshape(-1) for e in ref64.band_rel_err(O.forward(plan, x), ref, True)), _band_labels(plan, 1), full_table=True)
    P, _ = one_block_inputs(plan, n)
    ref = ref64.inverse(plan, P, n)
    y = dec([p.cuda() for p in P], n).cpu()
    b2, _ = _judge("inverse", "D one block", ref64.rel_err(y, ref, keep=(0,)), ref64.rel_err(O.inverse(plan, P, n), ref, keep=(0,)),
                   _block_labels(plan), full_table=True)
    assert not bad + b2, "\n".join(bad + b2)


def test_inverse_of_a_with_the_twin_is_at_fp32_rounding_of_float64():
    """``dc_twins`` and ``long_bands`` together: against ``ref64.inverse(..., twins=True)``, the reference's operation."""
    base, enc, dec = _fb("A", dc_twins=True)
    plan = oracle_plan("A")
    assert base.plan.dc_twins and base.plan.long_bands and len(plan.twins) == 1
    n = lengths(plan)[0]
    P, _ = one_block_inputs(plan, n)
    ref = ref64.inverse(plan, P, n, twins=True)
    y = dec([p.cuda() for p in P], n).cpu()
    bad, _ = _judge("inverse", "A one block, with the twin", ref64.rel_err(y, ref, keep=(0,)),
                    ref64.rel_err(O.inverse(plan, P, n, twins=True), ref, keep=(0,)), _block_labels(plan))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key", list(PLANS))
def test_masked_inverse_is_at_fp32_rounding_of_float64(key):
    """``backward_masked`` (tests/test_dc_twins_gpu.py): BC = 8 mask channels over BCx = 2 mix channels at S = 3, BC = 3 over BCx = 1 at
    S = 5, and a mask row per mix row (BC = BCx = 1 and 3) at both lengths."""
    base, enc, dec = _fb(key)
    eng, plan = base.nsgt, oracle_plan(key)
    bad = []
    for li, BC, BCx in ((0, 8, 2), (1, 3, 1), (0, 1, 1), (0, 3, 3), (1, 1, 1)):
        n, S = lengths(plan)[li], (3, 5)[li]
        gen = torch.Generator().manual_seed(n + BC)
        mix = [torch.randn(BCx, F, S, T, 2, generator=gen) for (_, F, T) in plan.blocks]
        masks = [torch.rand(BC, F, S, T, generator=gen) for (_, F, T) in plan.blocks]
        X = [mk[..., None] * mx.repeat(BC // BCx, 1, 1, 1, 1) for mk, mx in zip(masks, mix)]
        ref = ref64.inverse(plan, X, n)
        out = torch.empty(BC, n, dtype=torch.float32, device="cuda")
        offs = (torch.arange(BC, dtype=torch.int64) * n).cuda()
        eng.backward_masked(torch.cat([m.reshape(-1) for m in masks]).cuda(), torch.cat([m.reshape(-1) for m in mix]).cuda(), BC, BCx, S, n, out, offs)
        b, _ = _judge("inverse_masked", f"{key} n {n} BC {BC} BCx {BCx}", ref64.rel_err(out.cpu(), ref, keep=(0,)),
                      ref64.rel_err(O.inverse(plan, X, n), ref, keep=(0,)), [f"row {r}" for r in range(BC)])
        bad += [f"{key} n {n} BC {BC} BCx {BCx} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- 3. both adjoints, and autograd through both transforms ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(PLANS))
def test_both_adjoints_are_at_fp32_rounding_of_float64_autograd(key):
    """n = 2 h + 1 and 7 h + 123 with BC = 1 and 3, against float64 autograd through ref64; E: the closed forms of
    tests/test_autograd_cpu.py and tests/test_sdr_cpu.py in fp32."""
    base, enc, dec = _fb(key)
    eng, plan = base.nsgt, oracle_plan(key)
    bad = []
    for li, BC in SHAPES:
        n, S = lengths(plan)[li], (3, 5)[li]
        G64 = random_cotangents(plan, BC, S, seed=BC * 1000 + n % 997)
        ref = autograd_forward_adjoint(plan, G64, n)
        G32 = [g.float() for g in G64]
        cpu = forward_adjoint_closed_form(plan, G32, n, dtype=F32)
        got = eng.forward_adjoint(torch.cat([b.reshape(-1) for b in G32]).cuda(), (BC,), n)
        assert got.shape == (BC, n) and bool(torch.isfinite(got).all())
        b, _ = _judge("fwd_adjoint", f"{key} n {n} BC {BC}", ref64.rel_err(got.cpu(), ref, keep=(0,)), ref64.rel_err(cpu, ref, keep=(0,)),
                      [f"row {r}" for r in range(BC)])
        bad += [f"{key} fwd_adjoint n {n} BC {BC} {m}" for m in b]
        gy, ref, S2 = autograd_adjoint(plan, BC, n, seed=BC * 1000 + n % 997)
        assert S2 == S
        gy32 = gy.float()
        cpu = adjoint_closed_form(plan, adjoint_window(plan), gy32, S, dtype=F32)
        arena = eng.backward_adjoint(gy32.cuda(), S)
        got = [v.cpu() for v in eng.table.views(arena, (BC,), S)]
        b, _ = _judge("adjoint", f"{key} n {n} BC {BC}", _pair([ref64.rel_err(a, r) for a, r in zip(got, ref)]),
                      _pair([ref64.rel_err(c, r) for c, r in zip(cpu, ref)]), _block_labels(plan), full_table=(BC == 3 and li == 0))
        bad += [f"{key} adjoint n {n} BC {BC} {m}" for m in b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key", list(PLANS))
def test_reconstruction_and_its_gradient(key):
    """``insgt(nsgt(x))`` against float64 (and x itself at the contractual bar), and one ``backward()`` through both transforms against
    float64 autograd through ``ref64.inverse(ref64.forward(x))``; E: the same through the fp32 oracle."""
    base, enc, dec = _fb(key)
    plan = oracle_plan(key)
    bad = []
    for li, BC in SHAPES:
        n = lengths(plan)[li]
        x = audio(n, BC)
        w = torch.randn(BC, n, generator=torch.Generator().manual_seed(n + 3), dtype=F64)
        x64 = x.double().requires_grad_(True)
        y64 = ref64.inverse(plan, ref64.forward(plan, x64), n)
        (y64 * w).sum().backward()
        x32 = x.clone().requires_grad_(True)
        y32 = O.inverse(plan, O.forward(plan, x32), n)
        (y32 * w.float()).sum().backward()
        xd = x.cuda().requires_grad_(True)
        yd = dec(enc(xd), n)
        (yd * w.float().cuda()).sum().backward()
        assert yd.shape == (BC, n) and xd.grad is not None and xd.grad.shape == (BC, n)
        d = yd.detach().cpu().double() - y64.detach()
        assert float(d.pow(2).mean().sqrt()) < RMS_TOL and float(d.abs().max()) < MAX_TOL, (key, n, BC)
        for tag, got, cpu, ref in (("y", yd.detach().cpu(), y32.detach(), y64.detach()), ("grad", xd.grad.cpu(), x32.grad, x64.grad)):
            b, _ = _judge("roundtrip", f"{key} {tag} n {n} BC {BC}", ref64.rel_err(got, ref, keep=(0,)), ref64.rel_err(cpu, ref, keep=(0,)),
                          [f"row {r}" for r in range(BC)])
            bad += [f"{key} {tag} n {n} BC {BC} {m}" for m in b]
    assert not bad, "\n".join(bad)


# ---- 4. the reference's own numbers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(PLANS))
def test_transforms_equal_the_reference_fixture(key):
    """tests/golden/logscale*.npz with ``dc_twins=True`` (A and C: one twin; B: none): coefficients and decode at 1e-4 RMS / 1e-3
    max-abs."""
    from xumx_slicq_amd.synth import synth_audio
    base, enc, dec = _fb(key, dc_twins=True)
    g = load_golden("logscale.npz")
    n = int(g[f"n_{key}"])
    C = enc(synth_audio(n, seed=20260101 + n).cuda())
    assert len(C) == len(base.plan.blocks)
    for i, cb in enumerate(C):
        d = cb.cpu().double() - torch.from_numpy(g[f"fwd_{key}_{i}"]).double()
        rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
        print(f"[fixture] {key} fwd block {i}: rms {rms:.2e} max {mx:.2e}")
        assert rms < RMS_TOL and mx < MAX_TOL, (key, i, rms, mx)
    d = dec(C, n).cpu().double() - torch.from_numpy(g[f"inv_{key}"]).double()
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    _T.record("fixture", f"{key} inv", {"M_key": "fixture (absolute distance from the reference's decode; bar 1e-4 RMS / 1e-3 max)", "worst_ratio": mx / MAX_TOL,
                                        "rms": rms, "max": mx})
    assert rms < RMS_TOL and mx < MAX_TOL, (key, rms, mx)


@pytest.mark.parametrize("sk", list(G.STRATEGIES))
@pytest.mark.parametrize("key", list(PLANS))
def test_ideal_oracle_equals_the_reference_fixture(key, sk):
    """The reference's ``ideal_slicqt`` and ``_fast_sdr``: estimates at 1e-4 RMS / 1e-3 max-abs, SDRs within 1e-3 dB (the bars of
    tests/test_slicqfinder_gpu.py).  On C the T = 6416 block gives the Wiener filter four 5000-frame windows at S = 3."""
    from xumx_slicq_amd import scoring
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    g = load_golden("logscale.npz")
    n = int(g[f"n_{key}"])
    src = torch.from_numpy(G.case_sources(n))[:, None].contiguous().cuda()                  # (4, 1, 2, n)
    est = ideal_slicqt(src, _fb(key, dc_twins=True)[0], G.STRATEGIES[sk])
    ref = torch.from_numpy(np.stack([g[f"est_{key}_{sk}_{j}"] for j in range(4)]))[:, None]
    d = est.cpu() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    res = scoring.score(est, src, target_order=G.SOURCES, estimate_order=G.SOURCES)["targets"]
    sdr = np.asarray([res[t]["sdr_global"][0] for t in G.SOURCES])
    want = g[f"sdr_{key}_{sk}"]
    print(f"\n{key} {sk}: rms {rms:.3e} max {mx:.3e}; sdr diff {np.abs(sdr - want).max():.3e} dB")
    _T.record("fixture", f"ideal {key} {sk}", {"M_key": "fixture (absolute distance from the reference's decode; bar 1e-4 RMS / 1e-3 max)",
                                              "worst_ratio": mx / MAX_TOL, "rms": rms, "max": mx, "sdr_diff_db": float(np.abs(sdr - want).max())})
    assert bool(torch.isfinite(est).all())
    assert rms < RMS_TOL and mx < MAX_TOL, (rms, mx)
    assert np.abs(sdr - want).max() < 1e-3, (sdr, want)


def test_a_silent_stem_is_exactly_zero():
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    g = load_golden("logscale.npz")
    n = int(g["n_C"])
    src = torch.from_numpy(G.case_sources(n))[:, None].contiguous()
    src[2] = 0.0
    for sk in G.STRATEGIES.values():
        est = ideal_slicqt(src.cuda(), _fb("C")[0], sk)
        assert not bool(est[2].any()) and bool(est[0].any()) and bool(torch.isfinite(est).all()), sk
    base, enc, dec = _fb("C")
    C = enc(torch.zeros(1, 2, n).cuda())
    assert not any(bool(c.any()) for c in C) and not bool(dec(C, n).any())


# ---- 5. the spectrogram of C ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flatten", [False, True])
def test_spectrogram_db_of_c_against_float64(flatten):
    """The float64 restatement of tests/test_spectrogram_cpu.py on the device's own coefficients, by the rule of
    tests/test_spectrogram_gpu.py (E: the same steps in fp32 torch on the CPU); and ``spectrogram`` returns a finite image."""
    from test_spectrogram_gpu import TINY, cpu32_db
    from xumx_slicq_amd.visualization import blockwise_db, overlap_add_slicq, spectrogram
    base, enc, dec = _fb("C")
    plan = base.plan
    n, B = lengths(plan)[1], 1
    x = (0.1 * torch.randn(B, 2, n, generator=torch.Generator().manual_seed(n))).cuda()
    with torch.no_grad():
        X = enc(x)
    host = [torch.view_as_complex(b.cpu().contiguous()).numpy() for b in X]
    N = ref_columns(plan.blocks, plan.L, n, plan.num_slices(n), flatten)
    got = [d.cpu().numpy() for d in blockwise_db(X, n, base, flatten=flatten)]
    e_gpu, e_cpu, labels = [], [], []
    for k, (c, d, Nb) in enumerate(zip(host, got, N)):
        want, mag = ref_block_db(c, Nb, flatten), ref_block_magnitude(c, Nb, flatten)
        keep = ~((mag == 0.0).any(axis=1)) & ~(((mag != 0.0) & (mag < TINY)).any(axis=1))
        assert d.shape == want.shape and np.isfinite(d[keep]).all()
        cpu = cpu32_db(c, want.shape[-1], flatten)
        e_gpu.append(float(np.abs(d[keep] - want[keep]).max()) if keep.any() else 0.0)
        e_cpu.append(float(np.abs(cpu[keep] - want[keep]).max()) if keep.any() else 0.0)
        labels.append(f"block {k} T={plan.blocks[k][2]}")
    bad, _ = _judge("spectrogram/db", f"C n={n} flatten={flatten}", (e_gpu, e_gpu), (e_cpu, e_cpu), labels)
    assert not bad, bad
    ola = overlap_add_slicq(torch.view_as_complex(X[-1].contiguous()), flatten=flatten)
    assert ola.dtype == torch.complex64 and bool(torch.isfinite(torch.view_as_real(ola)).all())
    if not flatten:
        sp = spectrogram(x, base, width=256)
        assert tuple(sp.image.shape) == (B, plan.nbands, 256) and bool(torch.isfinite(sp.image).all()) and np.isfinite(sp.vmax).all()
        assert sp.freqs.shape == (plan.nbands,) and sp.freqs[0] == 0.0 and abs(sp.freqs[1] - 20.0) < 1e-3 and sp.freqs[-1] == 22050.0


# ---- 6. the search ---------------------------------------------------------------------------------------------------------------------------
def test_track_evaluator_scores_cqlog_with_the_keyword_and_refuses_without():
    from test_slicqfinder_gpu import tiny_dataset
    from xumx_slicq_amd.slicqfinder import TrackEvaluator
    ev = TrackEvaluator(tiny_dataset(), long_bands=True)
    got = ev.oracle("cqlog", 130.0, 10)
    assert len(got) == 4 and all(np.isfinite(got)) and ev.refusals == []
    assert ev.oracle("cqlog", 6.0, 14) == (float("-inf"),) * 4 and "plan refused" in ev.refusals[-1]["reason"] and "21440" in ev.refusals[-1]["reason"]
    ev0 = TrackEvaluator(tiny_dataset())
    assert ev0.oracle("cqlog", 130.0, 10) == (float("-inf"),) * 4
    assert "plan refused" in ev0.refusals[-1]["reason"] and "long_bands" in ev0.refusals[-1]["reason"]


# ---- 7. the same bits again, and on another stream ------------------------------------------------------------------------------------------
def test_second_call_and_non_default_stream_give_the_same_bits():
    base, enc, dec = _fb("C")
    plan = oracle_plan("C")
    n = lengths(plan)[1]
    x = audio(n, 3).cuda()
    C1 = [c.clone() for c in enc(x)]
    y1 = dec(C1, n).clone()
    C2 = enc(x)
    assert all(torch.equal(a, b) for a, b in zip(C1, C2)) and torch.equal(dec(C2, n), y1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        C3 = enc(x)
        y3 = dec(C3, n)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(C1, C3)) and torch.equal(y3, y1)


# ---- 8. the tables stay linear ----------------------------------------------------------------------------------------------------------------
def test_device_plan_of_cqlog_48_takes_less_than_64_mb():
    """21 long bands, Lg up to 5004: linear tables come to a few MB where the dense engine's matrices would take 3.7 GB.  A cap, not a
    measurement."""
    from xumx_slicq_amd.transforms import NSGTBase
    base = NSGTBase("cqlog", 48, 32.9, device="cuda", long_bands=True)
    assert int((base.plan.Lg > 320).sum()) == 21
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    base.nsgt.handle(dev)
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info()[0]
    print(f"device plan of cqlog, 48, 32.9: {used / 2 ** 20:.2f} MB")
    assert _num_long(base.nsgt) == 21 and used < 64 * 2 ** 20, used
    base.nsgt.close()
