"""Plans with bands across DC, opt-in (``build_plan(dc_twins=True)``, ``xsq_plan_create_twins``): the plan layer and the C ABI.
No GPU.  The device arithmetic is held in tests/test_dc_twins_gpu.py.

A band j >= 1 with 0 < c_j < Lg_j / 2 is synthesised a second time by the reference's inverse, through its negative-frequency
mirror (nsgt/nsigtf.py:57-99, quirk A12; ``oracle.slicqt.Plan.twins``).  By default the library refuses a plan on which that
term weighs TWIN_SHARE_MAX or more; with the flag it computes the term instead.  The survey below is over the default ranges of
``python -m xumx_slicq_amd.slicqfinder``: 60 of its first 200 draws have such a band; on 39 of them the term weighs 0.08 .. 0.32
and the default refuses the plan, on the other 21 it weighs 0.0026 .. 0.0084 and the default drops it by contract, as on Mel-32.
"""
import ctypes

import numpy as np
import pytest

from conftest import ROOT
from oracle import slicqt as O
from test_ref64_plans_cpu import PLANS

TWIN_PLANS = {"T": PLANS["T"], "K": PLANS["K"], "bark96": ("bark", 96, 32.9), "mel32": ("mel", 32, 115.5)}
REFUSED_BY_DEFAULT = ("T", "K", "bark96")
SURVEY = dict(seed=42, n_iter=200, scales=("bark", "mel"), bins=(10, 300), fmins=(10.0, 130.0, 0.1))      # the CLI's defaults
SURVEY_REFUSED, SURVEY_WITH_TWINS = 39, 60


def test_default_build_plan_still_refuses_with_todays_message():
    from xumx_slicq_amd.plan import TWIN_SHARE_MAX, build_plan
    with pytest.raises(ValueError) as e:
        build_plan(*PLANS["T"])
    msg = str(e.value)
    assert msg.startswith("plan (bark, 28, 32.9): band 1 (centre bin 2, Lg 16) reaches across DC and the reference's mirrored synthesis of it, "
                          "which the kernels do not compute, is 0.317 of the band's own")
    assert msg.endswith(f"(limit {TWIN_SHARE_MAX}): the stems would differ from the reference's")
    with pytest.raises(ValueError, match="reaches across DC"):
        build_plan(*PLANS["T"], dc_twins=False)


@pytest.mark.parametrize("name", list(TWIN_PLANS))
def test_flagged_plan_equals_the_oracles(name):
    """L, Lg, c, windows and blocks of ``oracle.slicqt.make_plan``, and ``twins`` equal to the oracle's tuples exactly: band, q,
    landing bins and the fp64 dual window of the MIRRORED band (not gd_j[Lg_j - q], which is equal to fp32 rounding of g only)."""
    from xumx_slicq_amd.plan import build_plan
    p, o = build_plan(*TWIN_PLANS[name], dc_twins=True), O.make_plan(*TWIN_PLANS[name])
    assert p.dc_twins is True
    assert (p.L, p.tr, p.nbands) == (o.L, o.tr, o.nbands)
    assert np.array_equal(p.Lg, o.Lg) and np.array_equal(p.c, o.c) and p.blocks == o.blocks
    assert np.array_equal(p.g, np.concatenate(o.g)) and np.array_equal(p.gd, np.concatenate(o.gd)) and np.array_equal(p.tw, o.tw)
    assert len(p.twins) == len(o.twins) >= 1
    for (j, q, k, gdm), (oj, oq, ok, ogdm) in zip(p.twins, o.twins):
        assert j == oj and np.array_equal(q, oq) and np.array_equal(k, ok)
        assert gdm.dtype == np.float64 and np.array_equal(gdm, ogdm)
        assert np.array_equal(k, q - int(p.c[j])) and q[0] == p.c[j] and q[-1] == p.Lg[j] // 2 - 1
    if name in ("T", "K"):
        assert [(t[0], t[1].tolist(), t[2].tolist()) for t in p.twins] == [(1, [2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5]), (2, [6, 7], [0, 1])]


def test_mel32_is_accepted_either_way_and_carries_its_twin_only_with_the_flag():
    from xumx_slicq_amd.plan import build_plan
    a, b = build_plan(*TWIN_PLANS["mel32"]), build_plan(*TWIN_PLANS["mel32"], dc_twins=True)
    assert a.dc_twins is False and a.twins == [] and [t[0] for t in b.twins] == [1]
    for f in ("L", "tr", "blocks"):
        assert getattr(a, f) == getattr(b, f)
    for f in ("Lg", "c", "g", "gd", "tw"):
        assert np.array_equal(getattr(a, f), getattr(b, f))


def test_bark262_with_the_flag_is_the_default_plan():
    from xumx_slicq_amd.plan import build_plan
    a, b = build_plan(), build_plan(dc_twins=True)
    assert b.twins == [] and a.twins == [] and b.dc_twins and not a.dc_twins
    assert (a.scale, a.fbins, a.fmin, a.fmax, a.fs, a.L, a.tr, a.blocks) == (b.scale, b.fbins, b.fmin, b.fmax, b.fs, b.L, b.tr, b.blocks)
    for f in ("Lg", "c", "g", "gd", "tw"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f


def test_new_symbols_are_declared_and_exported():
    from xumx_slicq_amd import _lib
    header = open(f"{ROOT}/include/xumx_slicq_hip.h").read()
    for sym in ("xsq_plan_create_twins", "xsq_plan_num_twins"):
        assert f"{sym}(" in header and hasattr(_lib.lib, sym) and sym in _lib._SIGS
    assert "#define XSQ_ABI_VERSION 2 " in header and _lib.lib.xsq_abi_version() == 2
    assert _lib.lib.xsq_plan_num_twins(None) < 0


def test_create_twins_rejects_null_arguments():
    from xumx_slicq_amd import _lib
    o = O.make_plan(*PLANS["T"])
    Lg, c = o.Lg.astype(np.int32), o.c.astype(np.int32)
    g, gd, tw = np.concatenate(o.g).astype(np.float32), np.concatenate(o.gd), o.tw.astype(np.float32)
    rc = _lib.lib.xsq_plan_create_twins(None, o.L, o.tr, len(Lg), Lg.ctypes.data, c.ctypes.data, g.ctypes.data, gd.ctypes.data, tw.ctypes.data)
    assert rc < 0 and "xsq_plan_create_twins" in _lib.last_error() and "null" in _lib.last_error()
    handle = ctypes.c_void_p()
    rc = _lib.lib.xsq_plan_create_twins(ctypes.byref(handle), o.L, o.tr, len(Lg), Lg.ctypes.data, c.ctypes.data, g.ctypes.data, None, tw.ctypes.data)
    assert rc < 0 and not handle.value and "null" in _lib.last_error()


def test_python_surface_takes_the_flag():
    """Signatures only (no device): every entry point the flag travels through has it, default False."""
    import inspect
    from xumx_slicq_amd import separator, slicqfinder, transforms
    from xumx_slicq_amd.plan import build_plan
    for fn in (build_plan, transforms.NSGTBase.__init__, separator.build_models, separator.load_target_models, separator.seeded_separator,
               separator.Separator.load, slicqfinder.TrackEvaluator.__init__):
        assert inspect.signature(fn).parameters["dc_twins"].default is False, fn
    args = slicqfinder.parse_args(slicqfinder.cli_parser(), ["--root", "x", "--dc-twins"])
    assert args.dc_twins is True and slicqfinder.parse_args(slicqfinder.cli_parser(), ["--root", "x"]).dc_twins is False
    seen = []
    res = slicqfinder.optimize_many(lambda scale, fmin, bins: seen.append((scale, bins, fmin)) or (1.0, 2.0, 3.0, 4.0),
                                    {"scales": ["bark"], "bins": (10, 300), "fmin": (10.0, 130.0, 0.1)}, 2, dc_twins=True)
    assert res["dc_twins"] is True and len(seen) == 2
    assert "dc_twins" not in slicqfinder.optimize_many(lambda scale, fmin, bins: (1.0, 2.0, 3.0, 4.0),
                                                       {"scales": ["bark"], "bins": (10, 300), "fmin": (10.0, 130.0, 0.1)}, 1)


def test_the_flag_opens_every_draw_of_the_default_search():
    """The first 200 draws of the CLI's default ranges, seed 42: with the flag all 200 build; the default refuses 39, each for a
    band across DC and for nothing else, and those 39 are exactly the draws whose twins weigh TWIN_SHARE_MAX or more.  (60 draws
    carry twins: the other 21 are accepted by default with the term dropped, as Mel-32 is.)  Fails without the feature."""
    from xumx_slicq_amd.plan import TWIN_SHARE_MAX, build_plan, dropped_twin_share
    from xumx_slicq_amd.slicqfinder import draw_params
    draws = draw_params(SURVEY["seed"], SURVEY["n_iter"], SURVEY["scales"], SURVEY["bins"], SURVEY["fmins"])
    assert len(draws) == 200
    with_twins, heavy, refused, shapes = [], [], [], set()
    for i, (scale, bins, fmin) in enumerate(draws):
        p = build_plan(scale, bins, fmin, dc_twins=True)
        if p.twins:
            with_twins.append(i)
            if float(dropped_twin_share(p.L, p.Lg, p.c, p.gd).max()) >= TWIN_SHARE_MAX:
                heavy.append(i)
            for (j, q, k, gdm) in p.twins:
                shapes.add((int(p.Lg[j]), int(p.c[j])))
            assert sum(len(t[1]) for t in p.twins) <= 8 and len(p.twins) <= 2 and p.L != 18060
        try:
            d = build_plan(scale, bins, fmin)
            assert d.twins == [] and np.array_equal(d.Lg, p.Lg) and np.array_equal(d.c, p.c) and np.array_equal(d.gd, p.gd)
        except ValueError as e:
            assert "reaches across DC" in str(e), (i, str(e))
            refused.append(i)
    print(f"draws with a band across DC: {len(with_twins)}, refused by default: {len(refused)}; (Lg, c) of those bands: {sorted(shapes)}")
    assert len(refused) == SURVEY_REFUSED and refused == heavy and len(with_twins) == SURVEY_WITH_TWINS
    assert {lg for lg, _ in shapes} == {16} and {c for _, c in shapes} <= {2, 4, 6}


# ---- the transpose of the mirrored synthesis, in closed form (the E of the GPU module's adjoint stage) --------------------------------
def twin_adjoint_closed_form(plan, gy, S, twins, dtype):
    """gy (BC, n) -> list over blocks of (BC, F_b, S, T_b, 2), zero outside the bands of ``twins``: the part of
    d <inverse(coef), gy> / d coef that the mirrored synthesis adds to ``adjoint_closed_form`` (tests/test_sdr_cpu.py), whose
    window a' has no term for it.  With V_s = rfft_L(gypad[(2s-2)h : (2s+2)h]) and w_k the irfft weights (1 at bins 0 and L/2,
    else 2):  g[s,j,t] += sign_j (-1)^q w_k Lg_j gd'_j[q] / L  (-+i) conj(V_s[q - c_j])  e^{+2 pi i (q + 1) t / Lg_j},
    -i on even slices, +i on odd ones."""
    import torch
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    L, h = plan.L, plan.h
    BC, n = gy.shape
    pad = torch.zeros(BC, (2 * S + 2) * h, dtype=dtype)
    pad[:, 2 * h: 2 * h + n] = gy.to(dtype)
    V = torch.fft.rfft(pad.unfold(-1, L, 2 * h)[:, :S])                                  # (BC, S, L/2 + 1)
    rot = torch.tensor([-1j if s % 2 == 0 else 1j for s in range(S)], dtype=cdt)
    out = [torch.zeros(BC, F, S, T, 2, dtype=dtype) for (_, F, T) in plan.blocks]
    for (j, q, k, gdm) in twins:
        b = max(i for i, (j0, _, _) in enumerate(plan.blocks) if j0 <= j)
        j0, F, T = plan.blocks[b]
        sign = 1.0 if (plan.c[j] // 2) % 2 == 0 else -1.0
        w = gdm * (T * sign / L) * np.where(q % 2 == 0, 1.0, -1.0) * np.where((k == 0) | (k == L // 2), 1.0, 2.0)
        A = V[:, :, torch.from_numpy(k)].conj() * rot[None, :, None] * torch.from_numpy(w).to(cdt)              # (BC, S, nq)
        ph = torch.exp(torch.from_numpy(2j * np.pi * np.outer(q + 1, np.arange(T)) / T)).to(cdt)              # (nq, T)
        out[b][:, j - j0] += torch.view_as_real(A @ ph)
    return out


@pytest.mark.parametrize("name", ["T", "K"])
def test_adjoint_closed_form_with_the_twin_term_equals_float64_autograd(name):
    """tests/test_ref64_plans_cpu.py shows that a' alone is NOT the adjoint of the reference's inverse on these plans (off by more
    than 1e-3); with the term above it is, to 1e-12 of the largest gradient."""
    import torch
    from test_ref64_plans_cpu import make_plan, n_for
    from test_sdr_cpu import adjoint_closed_form, adjoint_window, autograd_adjoint
    p = make_plan(name)
    n = n_for(p, 3)
    gy, ref, S = autograd_adjoint(p, 3, n, seed=5)
    own = adjoint_closed_form(p, adjoint_window(p), gy, S)
    twin = twin_adjoint_closed_form(p, gy, S, p.twins, torch.float64)
    without = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(own, ref))
    with_ = max(float((g + t - r).abs().max() / r.abs().max()) for g, t, r in zip(own, twin, ref))
    print(f"{name}: adjoint closed form against float64 autograd: without the twin term {without:.2e}, with it {with_:.2e}")
    assert without > 1e-3 and with_ <= 1e-12
