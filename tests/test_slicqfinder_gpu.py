"""The ideal-mask oracle on the device (xumx_slicq_amd/slicqfinder.py; xsq_ideal_separate, xsq_wiener_em_sources,
xsq_phasemix_sources) against the reference's own numbers (tests/golden/ideal_oracle*.npz, tools/make_golden_ideal.py), against
float64 (oracle/ref64.py restated with the same +5e-10 mix), and against itself where indexing goes wrong: bitwise identities
over shapes chosen for the edges -- n = 9031 (S = 3, mostly padding), n = 32768 on Mel-32 (many slices), windows with a ragged
last one, an odd window (the 8-byte path of the apply kernel), Mel-32, whose blocks are mostly single bands, and plan W
(``bark, 400, 300`` of tests/golden/plans3_W.npz) at its two-slice minimum.

Float64 rule (tests/test_ref64_gpu.py, oracle/parity.py): e_gpu <= M * E, E the error of the fp32 reference fixture (Bark-262,
Mel-32) or of the fp32 CPU oracle (plan W) against the same float64 result; one M per strategy, the smallest power of two at
least twice the worst ratio measured on MI355X (profiles/ref64_ideal.json), never above M_CAP.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle import model as omodel
from oracle import ref64
from oracle import slicqt as oslicqt
from oracle.parity import M_CAP, Tables

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_ideal", os.path.join(ROOT, "tools", "make_golden_ideal.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

PLANS = dict(G.PLANS, W=("bark", 400, 300.0))
# worst e_gpu / E measured on MI355X (profiles/ref64_ideal.json): wiener 0.80 (Bark-262), 0.05 (Mel-32), 0.96 (Mel-32, one window),
# 0.77 (W); phasemix 0.81, 0.12, 0.94 -> the smallest power of two at least twice the worst is 2 for both
M = {"ideal/wiener": 2, "ideal/phasemix": 2}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
TABLES = Tables("ref64_ideal", M)
EPS = 1.0e-10


@functools.lru_cache(maxsize=None)
def base_of(pk):
    from xumx_slicq_amd.transforms import NSGTBase
    return NSGTBase(*PLANS[pk], device="cuda")


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("ideal_oracle.npz")


def fixture_est(key):
    g = fixture()
    return torch.from_numpy(np.stack([g[f"est_{key}_{j}"] for j in range(4)]))


@functools.lru_cache(maxsize=None)
def sources_of(key):
    return torch.from_numpy(G.case_sources(key))[:, None].contiguous()          # (4, 1, 2, n)


def run(key, **kw):
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    pk, n, strategy, _, _ = G.CASES[key]
    if strategy == "chain":
        strategy, kw = "wiener", dict({"wiener_win_len": int(fixture()["win_len"])}, **kw)
    return ideal_slicqt(sources_of(key).cuda(), base_of(pk), strategy, **kw)


def oracle_cpu(plan, src, strategy, win, f64):
    """The oracle restated on the CPU oracle's stages, in float64 (oracle/ref64.py) or fp32 (oracle/slicqt.py, oracle/model.py):
    forward of the four sources -> mix = eps + sum_j (s_j + eps), magnitudes -> post-filter per block -> inverse.  (4, 1, 2, n)."""
    fwd, inv = (ref64.forward, ref64.inverse) if f64 else (oslicqt.forward, oslicqt.inverse)
    wien, pmix = (ref64.blockwise_wiener, ref64.phasemix_sep) if f64 else (omodel.blockwise_wiener, omodel.phasemix_sep)
    with torch.no_grad():
        C = fwd(plan, src.double() if f64 else src)
        Y = []
        for blk in C:                                    # (4, 1, 2, F, S, T, 2)
            mix = torch.full_like(blk[0], EPS)
            for j in range(4):
                mix = mix + (blk[j] + EPS)
            mag = torch.sqrt(blk[..., 0] ** 2 + blk[..., 1] ** 2)
            Y.append(wien(mix, mag, win) if strategy == "wiener" else pmix(mix, mag))
        return inv(plan, Y, src.shape[-1])


def compose(src, base, strategy, win):
    """The same oracle composed from the modules that existed before the one-call path."""
    from xumx_slicq_amd import phase
    from xumx_slicq_amd.transforms import ComplexNorm, make_filterbanks
    nsgt, insgt = make_filterbanks(base)
    C = nsgt(src)
    mags = ComplexNorm()(C)
    mix = [blk.sum(0) + 5 * EPS for blk in C]
    Y = phase.wiener(mix, mags, win) if strategy == "wiener" else phase.phasemix_sep(mix, mags)
    return insgt(Y, src.shape[-1])


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(G.CASES))
def test_estimates_and_sdrs_equal_the_reference_fixture(key):
    """Every fixture case: estimates at the project's contractual bar (1e-4 RMS, 1e-3 max-abs: BASELINE.json,
    tests/test_model_gpu.py), SDRs within 1e-3 dB; a silent stem exactly zero, the all-silent case exactly zero and finite."""
    from xumx_slicq_amd import scoring
    est = run(key)
    ref = fixture_est(key)[:, None]
    d = est.cpu() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    src = sources_of(key).cuda()
    res = scoring.score(est, src, target_order=G.SOURCES, estimate_order=G.SOURCES)["targets"]
    sdr = np.asarray([res[t]["sdr_global"][0] for t in G.SOURCES])
    want = fixture()[f"sdr_{key}"]
    print(f"\n{key}: rms {rms:.3e} max {mx:.3e}; sdr diff {np.abs(sdr - want).max():.3e} dB")
    assert bool(torch.isfinite(est).all())
    assert rms < 1e-4 and mx < 1e-3, (rms, mx)
    assert np.abs(sdr - want).max() < 1e-3, (sdr, want)
    for j, s in enumerate(G.CASES[key][3]):
        if s == 0:
            assert not bool(est[j].any()), f"stem {j} of {key} is silent in the reference"


# ---- against float64 ------------------------------------------------------------------------------------------------------
# (plan, strategy, window) -> the fixture case whose sources and fp32 estimates serve (None: seeded sources); E is the fixture's
# error where the fixture was made with that window, else the fp32 CPU oracle's.  Window 0 on Mel-32 at n = 32768: the longest
# rows have 7208 frames, so ONE window over all frames is another filter than the default 5000 gives.
F64_CASES = {("b", "wiener", 5000): "b9w", ("b", "phasemix", 5000): "b9p", ("m", "wiener", 5000): "m32w", ("m", "phasemix", 5000): "m32p",
             ("m", "wiener", 0): "m32w", ("W", "wiener", 5000): None, ("W", "phasemix", 5000): None}


@pytest.mark.parametrize("pk,strategy,win", list(F64_CASES))
def test_estimates_are_at_fp32_rounding_of_float64(pk, strategy, win):
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    from xumx_slicq_amd.synth import synth_audio
    key = F64_CASES[(pk, strategy, win)]
    plan = oslicqt.make_plan(*PLANS[pk])
    if key is not None:
        src = sources_of(key)
    else:
        src = torch.stack([g * synth_audio(9031, seed=50 + j) for j, g in enumerate((0.5, 0.35, 0.25, 0.4))])
    r64 = oracle_cpu(plan, src, strategy, win, True)
    cpu = fixture_est(key)[:, None] if key is not None and win == 5000 else oracle_cpu(plan, src, strategy, win, False)
    gpu = ideal_slicqt(src.cuda(), base_of(pk), strategy, win)
    e_gpu, e_cpu = ref64.rel_err(gpu, r64, keep=(0,)), ref64.rel_err(cpu, r64, keep=(0,))
    bad, worst = TABLES.judge("ideal", f"{PLANS[pk]} {strategy} win {win}", e_gpu, e_cpu, [f"stem {j}" for j in range(4)], arm=strategy)
    TABLES.dump()
    assert not bad, bad


# ---- bitwise identities ---------------------------------------------------------------------------------------------------
SHAPES = [("b", 9031, 5000), ("m", 32768, 50), ("m", 32768, 37), ("m", 9031, 0), ("m", 32768, 0), ("W", 9031, 5000)]


def seeded(n, B=1, seed=700):
    from xumx_slicq_amd.synth import synth_audio
    return torch.stack([g * synth_audio(n, seed=seed + j, nb_samples=B) for j, g in enumerate((0.5, 0.35, 0.25, 0.4))]).cuda()


@pytest.mark.parametrize("strategy", ["wiener", "phasemix"])
@pytest.mark.parametrize("pk,n,win", SHAPES)
def test_one_call_equals_the_three_abi_calls_and_in_place_equals_out_of_place(pk, n, win, strategy):
    from xumx_slicq_amd.slicqfinder import filter_sources_arena, ideal_slicqt
    base = base_of(pk)
    eng = base.nsgt
    src = seeded(n)
    one = ideal_slicqt(src, base, strategy, win)
    arena, lead, S = eng.forward(src)
    assert lead == (4, 1, 2)
    out = filter_sources_arena(eng.table, arena, torch.full_like(arena, float("nan")), 1, S, strategy, win)
    inplace = arena.clone()
    filter_sources_arena(eng.table, inplace, inplace, 1, S, strategy, win)
    assert bool(torch.isfinite(out).all())
    assert bits_equal(out, inplace), "in place differs from out of place"
    three = eng.backward(out, 8, S, n).view(4, 1, 2, n)
    assert bits_equal(one, three), "xsq_ideal_separate differs from forward -> filter -> inverse"
    assert bits_equal(one, ideal_slicqt(src, base, strategy, win)), "two runs differ"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ideal_slicqt(src, base, strategy, win)
    side.synchronize()
    assert bits_equal(one, other), "a non-default stream gives other bits"


@pytest.mark.parametrize("strategy", ["wiener", "phasemix"])
@pytest.mark.parametrize("pk,n,win", [("b", 9031, 5000), ("m", 32768, 50)])
def test_two_tracks_in_one_call_equal_two_calls(pk, n, win, strategy):
    """B = 2 with two DIFFERENT tracks, the second forty times louder: every item has its own window maximum."""
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    base = base_of(pk)
    src = seeded(n, B=2, seed=900)
    src[:, 1] *= 40.0
    both = ideal_slicqt(src, base, strategy, win)
    for b in range(2):
        assert bits_equal(both[:, b:b + 1].contiguous(), ideal_slicqt(src[:, b:b + 1].contiguous(), base, strategy, win)), f"item {b}"


@pytest.mark.parametrize("strategy", ["wiener", "phasemix"])
@pytest.mark.parametrize("pk,n,win", [("m", 32768, 50), ("m", 32768, 37), ("m", 9031, 0), ("m", 32768, 0), ("W", 9031, 5000)])
def test_equals_the_composition_of_the_public_modules(pk, n, win, strategy):
    """NSGT_SL -> ComplexNorm -> sum -> phase.wiener / phasemix_sep -> INSGT_SL gives the same estimates at the contractual bar;
    ``wiener_win_len`` = 0 means one window over all frames in both."""
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    base = base_of(pk)
    src = seeded(n, seed=1100)
    d = (ideal_slicqt(src, base, strategy, win) - compose(src, base, strategy, win)).cpu()
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    print(f"\n{pk} n={n} win={win} {strategy}: rms {rms:.3e} max {mx:.3e}")
    assert rms < 1e-4 and mx < 1e-3, (rms, mx)


# ---- argument checks ------------------------------------------------------------------------------------------------------
def test_window_zero_is_one_window_over_all_frames():
    """Mel-32 at n = 32768 (S = 34): the longest rows have 7208 frames, more than the default window of 5000.  ``wiener_win_len``
    = 0 gives the bits of a window as long as the longest row (one window in every block) and NOT those of 5000 (two windows in
    the long blocks); the arena-level call likewise.  (Held to float64 with one window above, and to the composed modules.)"""
    from xumx_slicq_amd.slicqfinder import filter_sources_arena, ideal_slicqt
    base = base_of("m")
    eng = base.nsgt
    src = seeded(32768, seed=1300)
    S = base.plan.num_slices(32768)
    longest = max(S * T for _, T in base.plan.block_shapes())
    assert longest == 7208 > 5000
    zero = ideal_slicqt(src, base, "wiener", 0)
    assert bits_equal(zero, ideal_slicqt(src, base, "wiener", longest)), "0 is not one window over all frames"
    assert not bits_equal(zero, ideal_slicqt(src, base, "wiener", 5000)), "0 was taken for the default window"
    arena, _, S2 = eng.forward(src)
    assert S2 == S
    a0 = filter_sources_arena(eng.table, arena, torch.empty_like(arena), 1, S, "wiener", 0)
    assert bits_equal(a0, filter_sources_arena(eng.table, arena, torch.empty_like(arena), 1, S, "wiener", longest))
    assert not bits_equal(a0, filter_sources_arena(eng.table, arena, torch.empty_like(arena), 1, S, "wiener", 5000))


def test_bad_arguments_raise():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    base = base_of("m")
    src = seeded(9031)
    with pytest.raises(_lib.XsqError, match="one EM iteration"):
        ideal_slicqt(src, base, niter=2)
    with pytest.raises(ValueError, match="four sources"):
        ideal_slicqt(src[:3].contiguous(), base)
    with pytest.raises(_lib.XsqError, match="ROCm device only"):
        ideal_slicqt(src.cpu(), base)
    with pytest.raises(ValueError):
        ideal_slicqt(src, base, strategy="softmask")
    # a shape that does not fit one launch: the workspace query answers 0 with the reason, and the call returns an error
    d = base.nsgt.demixer(src.device)
    assert _lib.lib.xsq_ideal_workspace(d, 30000, 9031, 0, 5000) == 0 and "exceed one launch" in _lib.last_error()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert _lib.lib.xsq_ideal_separate(d, src.data_ptr(), 30000, 9031, 0, 5000, src.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert _lib.lib.xsq_ideal_separate(d, src.data_ptr(), 1, 9031, 0, 5000, src.data_ptr(), ws.data_ptr(), 256, None) < 0
    assert "workspace too small" in _lib.last_error()


# ---- the evaluator --------------------------------------------------------------------------------------------------------
def tiny_dataset():
    from xumx_slicq_amd.data import DeviceDataset
    from xumx_slicq_amd.synth import synth_audio
    tracks = []
    for t, n in enumerate((20000, 14001)):
        tracks.append({s: (g * synth_audio(n, seed=300 + 10 * t + j)[0]).numpy()
                       for j, (s, g) in enumerate(zip(DeviceDataset.sources, (0.5, 0.35, 0.25, 0.4)))})
    return DeviceDataset.from_arrays(tracks, storage="fp32", device="cuda")


@pytest.mark.parametrize("piece", [None, 6000])
def test_track_evaluator_equals_the_hand_written_loop(piece):
    from xumx_slicq_amd import scoring
    from xumx_slicq_amd.slicqfinder import ORACLE_TARGETS, TrackEvaluator, ideal_slicqt
    ds = tiny_dataset()
    got = TrackEvaluator(ds, piece=piece).oracle("mel", 115.5, 32)
    base = base_of("m")
    per = {t: [] for t in ds.targets}
    for i in range(len(ds)):
        n = int(ds.lengths[i])
        if piece is None:
            (_, y), = list(ds.pieces(i, n))
            res = scoring.score(ideal_slicqt(y, base), y, target_order=ds.targets, estimate_order=ds.targets)
        else:
            sc = scoring.TrackScorer(1, n, target_order=ds.targets, estimate_order=ds.targets, device="cuda")
            for _, y in ds.pieces(i, piece):
                sc.add(ideal_slicqt(y, base), y)
            res = sc.result()
        for t in ds.targets:
            per[t].append(res["targets"][t]["sdr_global"][0])
    want = tuple(float(np.mean(per[t])) for t in ORACLE_TARGETS)
    assert got == want, (got, want)
    assert all(np.isfinite(got))


def test_refused_plans_and_long_slices_give_minus_inf_and_are_named():
    from xumx_slicq_amd.slicqfinder import TrackEvaluator
    ev = TrackEvaluator(tiny_dataset(), max_sllen=44100)
    inf4 = (float("-inf"),) * 4
    assert ev.oracle("bark", 32.9, 28) == inf4                  # a band across DC (tests/test_ref64_plans_cpu.py: plan T)
    assert ev.oracle("cqlog", 30.0, 100) == inf4                # not a scale plan.build_plan builds
    short = TrackEvaluator(tiny_dataset(), max_sllen=1000)
    assert short.oracle("mel", 115.5, 32) == inf4               # sllen 2016
    assert short.refusals == [{"scale": "mel", "bins": 32, "fmin": 115.5, "reason": "sllen 2016 > max_sllen 1000"}]
    assert [r["scale"] for r in ev.refusals] == ["bark", "cqlog"] and all("plan refused" in r["reason"] for r in ev.refusals)


def test_optimize_many_returns_the_best_of_its_own_rounds(tmp_path):
    import json
    from xumx_slicq_amd.slicqfinder import TrackEvaluator, optimize_many
    ev = TrackEvaluator(tiny_dataset(), tracks=[1])
    seen = []

    def f(**kw):
        seen.append(ev.oracle(**kw))
        return seen[-1]

    out = str(tmp_path / "search.json")
    # (these ranges reach down to plans with a band across DC: several draws of the table are refused before the third is scored)
    res = optimize_many(f, {"scales": ["bark", "mel"], "bins": (24, 40), "fmin": (30.0, 130.0, 0.5)}, 3, seed=7, out=out, refusals=ev.refusals)
    scored = [s for s in seen if s[0] != float("-inf")]
    assert len(res["rounds"]) == 3 == len(scored)
    assert res["rerolled"] == len(seen) - 3 == len(res["refusals"]) == len(ev.refusals) > 0
    assert [r["reason"] for r in res["refusals"]] == [r["reason"] for r in ev.refusals] and all("plan refused" in r["reason"] for r in res["refusals"])
    assert json.load(open(out))["refusals"] == res["refusals"]
    assert res["best"]["total"]["sdr"] == max(sum(s) / 4 for s in scored)
    assert json.load(open(out))["best"]["total"]["sdr"] == res["best"]["total"]["sdr"]
