"""The logarithmic scales ``cqlog`` and ``vqlog`` and the ``long_bands`` keyword: the plan layer, the C ABI and the search's command
line.  Owns the plans, shapes and helpers of tests/test_logscale_gpu.py.

  A = ``cqlog, 10, 130.0`` (L 2348; Lg .. 452, 768, 1020: the smallest plan with long bands, 452 = 4 * 113, a prime)
  B = ``vqlog, 24, 40.0`` at fgamma 15 (L 11652; nine long bands 360 .. 2788; the DC band, 28, is wider than its neighbour, 16, and
      takes the flat-topped window)
  C = ``cqlog, 12, 20.0`` (L 13620; long bands 384, 724, 1372, 2596, 4668, 6416: m = 96, 181, 343, 649, 1167, 1604)

A and C have one band across DC with a share of 0.007: dropped by contract without ``dc_twins``, computed with it.  The reference's
numbers are in tests/golden/logscale*.npz (tools/make_golden_logscale.py).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle import slicqt as O


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_logscale", os.path.join(ROOT, "tools", "make_golden_logscale.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _tool()
PLANS = G.PLANS                                # key -> (scale, fbins, fmin, fgamma)
# D = ``cqlog, 15, 12.0`` (L 27056; Lg .. 8592, 11240: m = 2148 and 2810, the engine's largest FFT class, 8192 points), not in the fixture
CONFIGS = {**PLANS, "D": ("cqlog", 15, 12.0, 15.0)}
FACTS = {"A": (2348, [16, 16, 16, 28, 48, 80, 144, 256, 452, 768, 1020]),
         "B": (11652, [28, 16, 16, 16, 16, 16, 24, 32, 40, 52, 68, 92, 120, 160, 208, 272, 360, 476, 624, 820, 1080, 1420, 1872, 2440, 2788]),
         "C": (13620, [16, 16, 16, 32, 56, 108, 204, 384, 724, 1372, 2596, 4668, 6416])}
TOO_LONG = ("cqlog", 14, 6.0)                  # L 45796, longest band 21440: above the engine's 16384
_PKG, _ORC = {}, {}


def pkg_plan(key, dc_twins=False):
    from xumx_slicq_amd.plan import build_plan
    if (key, dc_twins) not in _PKG:
        scale, fbins, fmin, fgamma = CONFIGS[key]
        _PKG[key, dc_twins] = build_plan(scale, fbins, fmin, fgamma=fgamma, dc_twins=dc_twins, long_bands=True)
    return _PKG[key, dc_twins]


def oracle_plan(key) -> O.Plan:
    """The package plan's fields as an ``oracle.slicqt.Plan`` (a plain dataclass; ``oracle.make_plan`` refuses these scales), with
    the twins of the ``dc_twins`` build: ``inverse(..., twins=True)`` is the reference's operation, ``twins=False`` the default
    engine's (shares below TWIN_SHARE_MAX: ``twins=None`` drops them too)."""
    if key not in _ORC:
        p = pkg_plan(key, dc_twins=True)
        off = np.concatenate(([0], np.cumsum(p.Lg)))
        _ORC[key] = O.Plan(fs=p.fs, L=p.L, tr=p.tr, nbands=p.nbands, Lg=p.Lg.astype(np.int64), c=p.c.astype(np.int64),
                           g=[p.g[off[j]: off[j + 1]].copy() for j in range(p.nbands)], gd=[p.gd[off[j]: off[j + 1]].copy() for j in range(p.nbands)],
                           tw=p.tw.copy(), blocks=list(p.blocks), twins=[(j, np.asarray(q), np.asarray(k), np.asarray(w)) for (j, q, k, w) in p.twins])
    return _ORC[key]


def lengths(plan):
    """n = 2 h + 1 (S = 3) and n = 7 h + 123 (S = 5, ragged tail)."""
    h = plan.L // 4
    return [2 * h + 1, 7 * h + 123]


def audio(n, rows, seed=0):
    """(rows, n) float32: seeded synth_audio channels, each row scaled differently."""
    from xumx_slicq_amd.synth import synth_audio
    x = torch.cat([synth_audio(n, seed=20260101 + n + seed + i)[0] for i in range((rows + 1) // 2)])[:rows]
    return (x * torch.linspace(1.0, 0.4, rows)[:, None]).contiguous()


@pytest.mark.parametrize("key", list(PLANS))
def test_plans_equal_the_reference_integers_exactly_and_windows_to_the_bit(key):
    g = load_golden("logscale.npz")
    for dc in (False, True):
        p = pkg_plan(key, dc)
        assert p.long_bands and p.dc_twins == dc and (p.L, p.Lg.tolist()) == FACTS[key]
        assert p.L == int(g[f"L_{key}"]) and p.tr == int(g[f"tr_{key}"])
        assert np.array_equal(p.Lg, g[f"Lg_{key}"]) and np.array_equal(p.c, g[f"c_{key}"])
        assert p.g.dtype == np.float32 and p.gd.dtype == np.float64
        assert np.array_equal(p.g, g[f"g_{key}"]) and np.array_equal(p.gd, g[f"gd_{key}"])
    assert p.num_slices(int(g[f"n_{key}"])) == 3 and lengths(p)[0] == int(g[f"n_{key}"]) and p.num_slices(lengths(p)[1]) == 5
    assert len(pkg_plan(key, True).twins) == {"A": 1, "B": 0, "C": 1}[key] and pkg_plan(key, False).twins == []


def test_shares_across_dc_are_below_the_limit_and_b_has_the_flat_topped_dc_window():
    from xumx_slicq_amd.plan import TWIN_SHARE_MAX, dropped_twin_share
    d = pkg_plan("D")
    assert d.L == 27056 and d.Lg.tolist()[-4:] == [3044, 5204, 8592, 11240] and 8196 < 8592            # 2 m - 1 > 4096: the 8192-point class
    for key, want in (("A", 0.007), ("B", 0.0), ("C", 0.007), ("D", 0.0)):
        p = pkg_plan(key)
        share = float(dropped_twin_share(p.L, p.Lg, p.c, p.gd).max())
        assert abs(share - want) < 5e-4 and share < TWIN_SHARE_MAX, (key, share)
    b = pkg_plan("B")
    assert b.Lg[0] == 28 > b.Lg[1] == 16 and np.all(b.g[:4] == 1.0) and b.g[14] == 0.0        # plateau of ones, Hann edges (peak-at-0 storage)
    assert b.fgamma == 15.0 and pkg_plan("A").fgamma == 15.0


def test_fgamma_moves_only_the_variable_q_scale():
    from xumx_slicq_amd.plan import build_plan
    v0 = build_plan("vqlog", 24, 40.0, fgamma=0.0, long_bands=True, dc_twins=True)
    c0 = build_plan("cqlog", 24, 40.0, fgamma=0.0, long_bands=True, dc_twins=True)
    c15 = build_plan("cqlog", 24, 40.0, fgamma=15.0, long_bands=True, dc_twins=True)
    assert v0.L == c0.L == c15.L and np.array_equal(v0.Lg, c0.Lg) and np.array_equal(c0.gd, c15.gd) and np.array_equal(v0.gd, c0.gd)
    assert not np.array_equal(pkg_plan("B").Lg, v0.Lg)


@pytest.mark.parametrize("scale", ["cqlog", "vqlog"])
def test_the_default_refuses_the_new_scales_and_names_the_keyword(scale):
    from xumx_slicq_amd.plan import build_plan
    from xumx_slicq_amd.transforms import NSGTBase
    with pytest.raises(ValueError, match="long_bands=True"):
        build_plan(scale, 10, 130.0)
    with pytest.raises(ValueError, match="long_bands"):
        build_plan(scale, 10, 130.0, long_bands=False, dc_twins=True)
    with pytest.raises(ValueError, match="long_bands"):
        NSGTBase(scale, 10, 130.0, device="cpu")
    with pytest.raises(ValueError, match="not on the accelerated path"):
        build_plan("octave", 10, 130.0, long_bands=True)


@pytest.mark.parametrize("cfg", [("bark", 262, 32.9), ("mel", 32, 115.5)])
def test_bark_and_mel_under_the_keyword_are_the_default_plans_field_for_field(cfg):
    import dataclasses
    from xumx_slicq_amd.plan import build_plan
    a, b = build_plan(*cfg), build_plan(*cfg, long_bands=True)
    assert b.long_bands and not a.long_bands
    for f in dataclasses.fields(a):
        if f.name == "long_bands":
            continue
        va, vb = getattr(a, f.name), getattr(b, f.name)
        assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, f.name
    assert int(b.Lg.max()) <= 320                     # no band reaches the engine: the device plan launches what it did


def test_a_band_above_the_engine_maximum_is_refused_by_name_on_the_host_and_by_the_library(monkeypatch):
    import ctypes
    from xumx_slicq_amd import _lib, plan
    wmax = plan.long_band_max()
    assert wmax == _lib.lib.xsq_plan_long_band_max() >= 8192 and _lib.lib.xsq_plan_long_band_min() == plan.LONG_BAND_MIN == 320
    assert int(plan.build_plan("cqlog", 19, 10.0, long_bands=True).Lg.max()) == 14244 <= wmax        # the longest band of the search's usual draws
    with pytest.raises(ValueError, match=r"band 14 has Lg 21440.*long_bands"):
        plan.build_plan(*TOO_LONG, long_bands=True)
    # a few-bins log scale's Nyquist band can exceed half the slice, which the library has never taken: restated on the host as well
    with pytest.raises(ValueError, match=r"band 12 has Lg 12432, longer than half the slice \(12350\)"):
        plan.build_plan("cqlog", 12, 10.0, long_bands=True)
    # the library's own refusal, on the same tables (host arithmetic: it comes before anything reaches a device)
    monkeypatch.setattr(plan, "long_band_max", lambda: 1 << 30)
    p = plan.build_plan(*TOO_LONG, long_bands=True, dc_twins=True)
    h = ctypes.c_void_p()
    args = (ctypes.byref(h), p.L, p.tr, p.nbands, p.Lg.ctypes.data, p.c.ctypes.data, p.g.ctypes.data, p.gd.ctypes.data, p.tw.ctypes.data)
    assert _lib.lib.xsq_plan_create_flags(*args, 3) == -1 and h.value is None
    assert "band 14 has Lg=21440" in _lib.last_error() and "xsq_plan_long_band_max" in _lib.last_error()
    assert _lib.lib.xsq_plan_create_flags(*args, 8) == -1 and "unknown flags" in _lib.last_error()
    assert _lib.lib.xsq_plan_num_long_bands(None) < 0


def test_new_symbols_are_exported_and_declared():
    from xumx_slicq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    for n in ("xsq_plan_create_flags", "xsq_plan_long_band_max", "xsq_plan_long_band_min", "xsq_plan_num_long_bands"):
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTED and n + "(" in hdr, n
    assert "#define XSQ_PLAN_TWINS 1u" in hdr and "#define XSQ_PLAN_LONG_BANDS 2u" in hdr
    assert "#define XSQ_ABI_VERSION 2 " in hdr and _lib.lib.xsq_abi_version() == 2


def test_cli_parses_with_and_without_long_bands(capsys):
    from xumx_slicq_amd.slicqfinder import cli_parser, parse_args
    a = parse_args(cli_parser(), ["--root", "D"])
    assert not a.long_bands and a.fscale == "bark,mel" and a.params["scales"] == ["bark", "mel"]
    a = parse_args(cli_parser(), ["--root", "D", "--long-bands"])
    assert a.long_bands and a.fscale == "bark,mel,cqlog" and a.params["scales"] == ["bark", "mel", "cqlog"]
    a = parse_args(cli_parser(), ["--root", "D", "--long-bands", "--fscale", "vqlog,mel"])
    assert a.params["scales"] == ["vqlog", "mel"]
    a = parse_args(cli_parser(), ["--root", "D", "--long-bands", "--single", "--fscale", "cqlog", "--fbins", "12", "--fmins", "20"])
    assert a.single and a.params == {"scale": "cqlog", "bins": 12, "fmin": 20.0}
    for scale in ("cqlog", "vqlog"):
        with pytest.raises(SystemExit):
            parse_args(cli_parser(), ["--root", "D", "--fscale", scale])
        err = capsys.readouterr().err
        assert scale in err and "--long-bands" in err
    with pytest.raises(SystemExit):
        parse_args(cli_parser(), ["--root", "D", "--long-bands", "--fscale", "octave"])


def test_the_evaluator_and_nsgtbase_take_the_keyword():
    import inspect
    from xumx_slicq_amd.slicqfinder import TrackEvaluator, evaluate_single, optimize_many
    from xumx_slicq_amd.transforms import NSGTBase
    assert inspect.signature(TrackEvaluator.__init__).parameters["long_bands"].default is False
    assert inspect.signature(NSGTBase.__init__).parameters["long_bands"].default is False
    assert list(inspect.signature(NSGTBase.__init__).parameters)[1:8] == ["scale", "fbins", "fmin", "fmax", "fgamma", "fs", "device"]
    base = NSGTBase("vqlog", 24, 40.0, fgamma=15.0, device="cpu", long_bands=True)
    assert base.plan.long_bands and base.sllen == 11652 and base.M == 2788
    res = optimize_many(lambda **kw: (1.0, 2.0, 3.0, 4.0), {"scales": ["cqlog"], "bins": (10, 12), "fmin": (20.0, 30.0, 1.0)}, 2, seed=1, long_bands=True)
    assert res["long_bands"] is True and len(res["rounds"]) == 2
    assert evaluate_single(lambda **kw: (1.0, 2.0, 3.0, 4.0), {"scale": "cqlog", "bins": 12, "fmin": 20.0}, long_bands=True)["long_bands"] is True


def test_fixture_sdrs_are_the_global_sdr_of_its_own_estimates():
    from xumx_slicq_amd.evaluation import global_sdr
    g = load_golden("logscale.npz")
    for key in PLANS:
        src = G.case_sources(int(g[f"n_{key}"]))
        for sk in G.STRATEGIES:
            for j in range(4):
                est = g[f"est_{key}_{sk}_{j}"]
                assert est.shape == src[j].shape and est.dtype == np.float32
                assert abs(global_sdr(src[j].T, est.T) - g[f"sdr_{key}_{sk}"][j]) < 1e-3, (key, sk, j)
