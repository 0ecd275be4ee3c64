"""The Wiener filter's option sets (``softmask``, ``residual``), host side: the float64 / complex64 helper the GPU tests are judged
by against the reference-generated fixture (tests/golden/wiener_options.npz, tools/make_golden_wiener_options.py: per window
``norbert.wiener(contrib.residual_model(v, x, 1), x, k, use_softmask)``), and the host logic -- ``to_dict`` on five estimates, the
refusals that need no device, the command line, and the workspace / shape arithmetic of five sources."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64
from test_wiener_iters_cpu import wiener_iters

XSQ_ERR_ARG = -1
EPS = float(torch.finfo(torch.float32).eps)          # every epsilon of norbert is float32's, in the float64 arm too
CASES = ((1, 0, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 2), (0, 1, 3))        # (softmask, residual, niter)


def wiener_options(X, Ymag, niter, softmask=False, residual=False, win_len=omodel.WIENER_WIN, dtype=torch.complex128):
    """``wiener_iters`` (tests/test_wiener_iters_cpu.py) with the two options, as closed forms:
      residual   v_4 = relu(max(|x|, eps) - (((v_0 + v_1) + v_2) + v_3)) per channel (norbert/contrib.py:11-77, alpha = 1;
                 F.threshold replaces values <= eps), appended last;
      softmask   the start is x v_j / (eps + sum_j v_j) per channel over all sources (norbert/__init__.py:263-309) instead of
                 v_j exp(i angle x);
    then per window of the flattened (slice, time) axis ONE scaling by max(1, 0.1 max|x|) (over the batch too) around ``niter``
    applications of ``omodel._em_one_iteration`` (none, and no scaling, for ``niter`` = 0).  complex128: the float64 reference;
    complex64: the fp32 CPU comparand.  X (B,2,F,S,T,2), Ymag (4,B,2,F,S,T) -> (J,B,2,F,S,T,2), J = 4 + residual."""
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    B, Cc, Fb, S, T, _ = X.shape
    N = S * T
    x = torch.view_as_complex(X.to(real).reshape(B, Cc, Fb, N, 2).contiguous()).permute(0, 3, 2, 1)      # (B,N,F,C)
    v = Ymag.to(real).reshape(4, B, Cc, Fb, N).permute(1, 4, 3, 2, 0)                                     # (B,N,F,C,4)
    if residual:
        ax = x.abs()
        vx = torch.where(ax > EPS, ax, torch.full_like(ax, EPS))
        vr = (vx - (((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])).relu()
        v = torch.cat((v, vr[..., None]), dim=-1)
    J = v.shape[-1]
    wl = win_len if win_len else N
    y = torch.zeros(B, N, Fb, Cc, J, dtype=dtype)
    for p in range(0, N, wl):
        xw, vw = x[:, p:p + wl], v[:, p:p + wl]
        if softmask:
            yw = (vw / (EPS + vw.sum(-1, keepdim=True))) * xw[..., None]
        else:
            yw = vw * torch.exp(1j * torch.angle(xw[..., None]))
        if niter:
            max_abs = max(1.0, float(xw.abs().max()) * 0.1)
            yw, xs = yw / max_abs, xw / max_abs
            for _ in range(niter):
                yw = omodel._em_one_iteration(yw, xs)
            yw = yw * max_abs
        y[:, p:p + wl] = yw
    return torch.view_as_real(y).permute(4, 0, 3, 2, 1, 5).contiguous().reshape(J, B, Cc, Fb, S, T, 2)


def case_name(softmask, residual, niter):
    return f"s{int(softmask)}r{int(residual)}k{int(niter)}"


@pytest.fixture(scope="module")
def golden():
    return load_golden("wiener_options.npz")


# ---- 1. the helper against the reference ---------------------------------------------------------------------------------------------
def test_fixture_inputs_are_what_the_issue_asks_for(golden):
    X, m = torch.from_numpy(golden["X"]), torch.from_numpy(golden["masks"])
    assert X.shape == (2, 2, 2, 4, 39, 2) and m.shape == (4, 2, 2, 2, 4, 39) and int(golden["win_len"]) == 64
    assert sorted(map(tuple, golden["cases"].tolist())) == sorted(CASES)
    assert float(m.min()) > 0 and float(m.max()) < 0.5
    share = float((m.sum(0) > 1).float().mean())
    print(f"share of points with sum of masks > 1: {share:.3f}")
    assert 0.25 <= share <= 0.75                       # a residual that is zero everywhere or nowhere tests nothing
    mag = omodel.abs_of_real_complex(X).reshape(2, 2, 2, 156)
    both = (mag == 0).all(1).all(0).all(0)             # frames silent in both channels of every row and bin
    one = (mag[:, 1] == 0).all(0).all(0) & (mag[:, 0] > 0).all(0).all(0)
    assert int(both.sum()) == 1 and int(one.sum()) == 1
    assert float(mag[1].pow(2).mean().sqrt() / mag[0].pow(2).mean().sqrt()) > 30          # batch row 1 is forty times louder
    # the stored magnitudes are m |x| in fp32.  Not bit for bit on every host: re^2 + im^2 may or may not be contracted into an FMA
    # and the square root's vector path differs, one ulp each at the most, and the product rounds once more: 2.5 ulp = 3e-7
    Ymag, want = torch.from_numpy(golden["Ymag"]), m * omodel.abs_of_real_complex(X)
    assert Ymag.shape == want.shape and bool(((Ymag - want).abs() <= 3e-7 * want.abs()).all())
    assert bool((Ymag.reshape(4, 2, 2, 2, 156)[..., both] == 0).all())                   # and a silent frame has no magnitude at all


@pytest.mark.parametrize("softmask,residual,niter", CASES)
def test_helper_matches_the_reference_norbert(golden, softmask, residual, niter):
    """The complex64 arm of the helper against the reference's complex64 result, per source: at most 4 x the reference's own
    complex64-vs-complex128 spread for the case (stored by the generator; 4 x because the helper is a closed form, not the
    reference's einsum order).  The complex128 arm is what the complex64 one rounds: inside the same bound."""
    X, Ymag = torch.from_numpy(golden["X"]), torch.from_numpy(golden["Ymag"])
    name = case_name(softmask, residual, niter)
    ref, spread = torch.from_numpy(golden[f"Y_{name}"]), golden[f"spread_{name}"]
    J = 4 + residual
    assert ref.shape == (J, 2, 2, 2, 4, 39, 2) and spread.shape == (J,) and bool((spread > 0).all()) and bool(torch.isfinite(ref).all())
    for dtype in (torch.complex64, torch.complex128):
        got = wiener_options(X, Ymag, niter, bool(softmask), bool(residual), win_len=64, dtype=dtype)
        assert bool(torch.isfinite(got).all())
        rms, _ = ref64.rel_err(got, ref, keep=(0,))
        print(name, str(dtype), "rel rms per source", " ".join(f"{e:.2e}" for e in rms), "| spread", " ".join(f"{e:.2e}" for e in spread))
        assert bool((rms <= 4 * spread).all()), (name, dtype, rms, spread)


def test_fixture_cases_differ(golden):
    """The fixture can tell the option sets apart: the four targets of (softmask, k = 1) from those of (residual, k = 1), and the
    residual is a source of its own weight."""
    a, b = torch.from_numpy(golden["Y_s1r0k1"]), torch.from_numpy(golden["Y_s0r1k1"])
    assert float(ref64.rel_err(a, b[:4])[0]) > 1e-2
    assert float(b[4].pow(2).mean().sqrt() / b[:4].pow(2).mean().sqrt()) > 1e-2


# ---- 2. flags off -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [0, 1, 2])
def test_helper_with_both_flags_off_is_wiener_iters(golden, niter):
    X, Ymag = torch.from_numpy(golden["X"]), torch.from_numpy(golden["Ymag"])
    for wl in (64, 0):
        for dtype in (torch.complex64, torch.complex128):
            assert torch.equal(wiener_options(X, Ymag, niter, win_len=wl, dtype=dtype), wiener_iters(X, Ymag, niter, win_len=wl, dtype=dtype))


# ---- 3. host logic ------------------------------------------------------------------------------------------------------------------------
def test_to_dict_names_the_residual():
    from xumx_slicq_amd.separator import Separator
    est = torch.arange(5 * 2 * 3, dtype=torch.float32).reshape(5, 1, 2, 3)
    d = Separator.to_dict(est)
    assert list(d) == Separator.sources + ["residual"] and torch.equal(d["residual"], est[4]) and torch.equal(d["drums"], est[3])
    assert list(Separator.to_dict(est[:4])) == Separator.sources
    agg = Separator.to_dict(est, {"acc": ["bass", "other", "drums"], "rest": ["residual", "vocals"]})
    assert torch.equal(agg["rest"], est[4] + est[1])


def _cpu_separator():
    """A Separator around a small Unmix on the host: enough for the properties and the refusals that run before any device call."""
    from xumx_slicq_amd.model import Unmix
    from xumx_slicq_amd.separator import Separator
    sep = Separator.__new__(Separator)
    torch.nn.Module.__init__(sep)
    sep.xumx_model = Unmix([torch.zeros(1, 2, 2, 3, 4)])
    sep.chunk_size = 1000
    return sep


def test_options_live_on_the_model_and_default_off():
    from xumx_slicq_amd.model import Unmix
    sep = _cpu_separator()
    assert (sep.softmask, sep.residual, sep.niter) == (False, False, 1)
    assert Unmix([torch.zeros(1, 2, 2, 3, 4)]).wiener_options() == (0, 0)
    sep.softmask, sep.residual = 1, True
    assert sep.xumx_model.softmask is True and sep.xumx_model.residual is True and sep._nb_sources() == 5
    assert sep.xumx_model.wiener_options() == (1, 1)


def test_refusals_that_need_no_device():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.training import Trainer
    sep = _cpu_separator()
    sep.residual = True
    with pytest.raises(ValueError, match="residual"):
        sep.remix(torch.zeros(1, 2, 8), {"vocals": 0})
    with pytest.raises(ValueError, match="residual"):
        sep.demix_into(torch.zeros(1, 2, 8), torch.zeros(4, 1, 2, 8), torch.zeros(4, 1, 2, dtype=torch.int64))
    # a realtime (mix-phase-only) model has no Wiener filter to start or extend
    for opt in ("softmask", "residual"):
        rt = _cpu_separator()
        for blk in rt.xumx_model.sliced_umx:
            blk.realtime = True
        setattr(rt, opt, True)
        with pytest.raises(_lib.XsqError, match=opt):
            rt.forward(torch.zeros(1, 2, 8))
        with pytest.raises(_lib.XsqError, match=opt):
            rt.xumx_model.wiener_options()
    # the trainer differentiates the reference's filter only (its device check comes first: the option check needs cuda)
    for opt in ("softmask", "residual"):
        m = _cpu_separator().xumx_model
        setattr(m, opt, True)
        with pytest.raises(_lib.XsqError) as e:
            Trainer(m, (None, None, None), device="cuda")
        assert opt in str(e.value)


def test_options_of_the_command_line():
    from xumx_slicq_amd.inference import cli_parser, parse_args
    a = parse_args(cli_parser(), [])
    assert a.softmask is False and a.residual is False
    a = parse_args(cli_parser(), ["--softmask", "--residual", "--niter", "2"])
    assert a.softmask and a.residual and a.niter == 2
    assert parse_args(cli_parser(), ["--softmask", "--remix", "karaoke:vocals=0"]).softmask            # remix honours softmask
    for bad in (["--residual", "--remix", "karaoke:vocals=0"], ["--residual", "--realtime"], ["--softmask", "--realtime"]):
        with pytest.raises(SystemExit):
            parse_args(cli_parser(), bad)


def _tables(T=39):
    return np.asarray([2], dtype=np.int32), np.asarray([T], dtype=np.int32)


def test_workspace_and_shape_arithmetic_of_five_sources():
    """B = 2, F = 2, 156 frames in windows of 64: 4 rows x 3 windows.  The slot has 24 floats at J = 4 (unchanged: the training
    backward reads it) and 32 at J = 5; the iteration workspace adds one float per (block, item, window) and 256 bytes."""
    from xumx_slicq_amd import _lib, phase
    L = _lib.lib
    F, T = _tables()
    g = (1, F.ctypes.data, T.ctypes.data, 2, 4, 64)
    al = lambda n: (n + 255) // 256 * 256
    assert L.xsq_wiener_workspace(*g) == 4 * 3 * 24 * 4 + 256
    for flags, slot in ((0, 24), (phase.SOFTMASK, 24), (phase.RESIDUAL, 32), (phase.SOFTMASK | phase.RESIDUAL, 32)):
        for niter in (0, 1, 3):
            assert L.xsq_wiener_options_workspace(*g, niter, 0, flags) == al(4 * 3 * slot * 4 + 256) + 2 * 3 * 4 + 256
    assert L.xsq_wiener_options_workspace(*g, 1, 0, 0) == L.xsq_wiener_iter_workspace(*g, 1, 0)
    assert L.xsq_wiener_options_workspace(*g, 1, 0, 4) == 0 and L.xsq_wiener_options_workspace(*g, -1, 0, 2) == 0
    assert L.xsq_wiener_options_workspace(*g, 1, 3, 2) == 0
    assert phase.option_flags() == 0 and phase.option_flags(True, True) == 3 and phase.nb_sources(True) == 5 and phase.nb_sources() == 4
    # the resident bound: today's value by default, fewer frames per thread at five sources
    assert phase.resident_max_window() == phase.resident_max_window(4) == L.xsq_wiener_resident_max_window() >= 5000
    assert 0 < phase.resident_max_window(5) <= phase.resident_max_window(4) and phase.resident_max_window(5) % 1024 == 0
    with pytest.raises(ValueError):
        phase.resident_max_window(6)
    assert L.xsq_abi_version() == 2


def test_option_entry_points_check_their_arguments_without_a_device():
    from xumx_slicq_amd import _lib, phase
    L = _lib.lib
    F, T = _tables()
    buf = np.zeros(64, dtype=np.float32)
    p, big = buf.ctypes.data, 1 << 40
    g = (1, F.ctypes.data, T.ctypes.data)
    assert L.xsq_wiener_em_options(*g, p, p, 2, 4, 64, 0, 1, 0, 4, p, big, None) == XSQ_ERR_ARG and "flags" in _lib.last_error()
    assert L.xsq_wiener_em_masked_options(*g, p, p, p, 2, 4, 64, 0, None, -1, 0, 3, p, big, None) == XSQ_ERR_ARG and "niter" in _lib.last_error()
    assert L.xsq_wiener_em_masked_options(*g, p, p, p, 2, 4, 63, 0, None, 1, 0, 3, p, big, None) == XSQ_ERR_ARG and "even" in _lib.last_error()
    assert L.xsq_wiener_em_masked_options(*g, p, p, p, 2, 4, 64, 0, None, 1, 0, 2, p, 16, None) == XSQ_ERR_ARG and "workspace" in _lib.last_error()
    assert L.xsq_wiener_start(*g, p, p, p, 2, 4, 0, None) == XSQ_ERR_ARG and "flags" in _lib.last_error()
    # a window between the two resident bounds: method = 2 is refused at five sources only
    w5 = phase.resident_max_window(5)
    Fl, Tl = _tables(T=w5 // 2 + 2)
    gl = (1, Fl.ctypes.data, Tl.ctypes.data)
    rc = L.xsq_wiener_em_masked_options(*gl, p, p, p, 2, 2, w5 + 4, 0, None, 2, 2, phase.RESIDUAL, p, big, None)
    assert rc == XSQ_ERR_ARG and "resident" in _lib.last_error()
    assert math.ceil((w5 + 4) / 1024) * 1024 <= phase.resident_max_window(4)
