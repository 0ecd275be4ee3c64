"""More than one Wiener-EM iteration (``niter``), host side: the k-iteration helpers the GPU tests are judged by against the
reference-generated fixture (tests/golden/wiener_iters.npz, tools/make_golden_wiener_iters.py: the reference's
norbert.wiener(v, x, k, False) per window), the argument checks of the new C entry points (no device needed: they return
before any HIP call), the schedule and the command line."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64

XSQ_ERR_ARG = -1


def wiener_iters(X, Ymag, niter, win_len=omodel.WIENER_WIN, dtype=torch.complex128):
    """``ref64.blockwise_wiener`` with ``niter`` iterations: per window of the flattened (slice, time) axis ONE scaling by
    max(1, 0.1 max|x|) (over the batch too), ``niter`` applications of ``omodel._em_one_iteration``, and the scale back
    (norbert/__init__.py:247-260 around :133-148).  complex128: the float64 reference; complex64: the fp32 CPU comparand.
    X (B,2,F,S,T,2), Ymag (4,B,2,F,S,T) -> (4,B,2,F,S,T,2)."""
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    B, Cc, Fb, S, T, _ = X.shape
    N = S * T
    x = torch.view_as_complex(X.to(real).reshape(B, Cc, Fb, N, 2).contiguous()).permute(0, 3, 2, 1)      # (B,N,F,C)
    v = Ymag.to(real).reshape(4, B, Cc, Fb, N).permute(1, 4, 3, 2, 0)                                     # (B,N,F,C,J)
    wl = win_len if win_len else N
    y = torch.zeros(B, N, Fb, Cc, 4, dtype=dtype)
    for p in range(0, N, wl):
        xw, vw = x[:, p:p + wl], v[:, p:p + wl]
        yw = vw * torch.exp(1j * torch.angle(xw[..., None]))                                             # :250
        if niter:
            max_abs = max(1.0, float(xw.abs().max()) * 0.1)                                              # :257
            yw, xs = yw / max_abs, xw / max_abs
            for _ in range(niter):
                yw = omodel._em_one_iteration(yw, xs)
            yw = yw * max_abs
        y[:, p:p + wl] = yw
    return torch.view_as_real(y).permute(4, 0, 3, 2, 1, 5).contiguous().reshape(4, B, Cc, Fb, S, T, 2)


@pytest.fixture(scope="module")
def golden():
    return load_golden("wiener_iters.npz")


@pytest.mark.parametrize("k", [2, 3])
def test_fp32_helper_matches_the_reference_norbert(golden, k):
    """The fp32 helper (k applications of the oracle's iteration around one scaling) against the reference's
    norbert.wiener(v, x, k, False) per 250-frame window: relative RMS <= 2e-6 (measured 3.7e-7 and 4.4e-7)."""
    X, Ymag = torch.from_numpy(golden["X"]), torch.from_numpy(golden["Ymag"])
    assert X.shape == (2, 2, 2, 4, 153, 2) and int(golden["win_len"]) == 250
    ref = torch.from_numpy(golden[f"Y_k{k}"])
    got = wiener_iters(X, Ymag, k, win_len=250, dtype=torch.complex64)
    rms, _ = ref64.rel_err(got, ref)
    print(f"k={k}: rel rms {float(rms):.3e}")
    assert float(rms) <= 2e-6, float(rms)
    # and the float64 helper is what the fp32 one rounds: the same distance from the reference, to fp32 rounding
    rms64, _ = ref64.rel_err(wiener_iters(X, Ymag, k, win_len=250), ref)
    assert float(rms64) <= 2e-6, float(rms64)


def test_fixture_iterations_differ(golden):
    """The fixture can tell k = 2 from k = 3 (and a helper that ignored k would fail above)."""
    rms, _ = ref64.rel_err(torch.from_numpy(golden["Y_k2"]), torch.from_numpy(golden["Y_k3"]))
    assert float(rms) > 1e-2


def test_float64_helper_with_one_iteration_is_ref64(golden):
    X, Ymag = torch.from_numpy(golden["X"]), torch.from_numpy(golden["Ymag"])
    for wl in (250, 0):
        assert torch.equal(wiener_iters(X, Ymag, 1, win_len=wl), ref64.blockwise_wiener(X, Ymag, win_len=wl))
    assert float(ref64.rel_err(wiener_iters(X, Ymag, 0), ref64.phasemix_sep(X, Ymag))[0]) < 1e-15      # k = 0: mix-phase


def _tables(T=153):
    return np.asarray([2], dtype=np.int32), np.asarray([T], dtype=np.int32)


def test_resident_window_bound_covers_the_default_window():
    from xumx_slicq_amd import _lib
    assert _lib.lib.xsq_wiener_resident_max_window() >= 5000


def test_iteration_entry_points_check_their_arguments_without_a_device():
    """Negative niter, an odd window on the masked entry point and method = 2 with a window above the resident bound are
    XSQ_ERR_ARG before any HIP call (the pointers are never followed: a dummy host buffer stands for all of them)."""
    from xumx_slicq_amd import _lib
    L = _lib.lib
    F, T = _tables()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    big = 1 << 40
    S = 4
    assert L.xsq_wiener_em_iter(1, F.ctypes.data, T.ctypes.data, p, p, 2, S, 250, 0, -1, 0, p, big, None) == XSQ_ERR_ARG
    assert "niter" in _lib.last_error()
    assert L.xsq_wiener_em_masked_iter(1, F.ctypes.data, T.ctypes.data, p, p, p, 2, S, 250, 0, None, -3, 0, p, big, None) == XSQ_ERR_ARG
    assert "niter" in _lib.last_error()
    assert L.xsq_wiener_em_masked_iter(1, F.ctypes.data, T.ctypes.data, p, p, p, 2, S, 251, 0, None, 2, 0, p, big, None) == XSQ_ERR_ARG
    assert "even" in _lib.last_error()
    assert L.xsq_wiener_em_iter(1, F.ctypes.data, T.ctypes.data, p, p, 2, S, 250, 0, 2, 3, p, big, None) == XSQ_ERR_ARG
    assert "method" in _lib.last_error()
    # a window above the bound: rows of S * T frames with win_len beyond them, and win_len itself
    wmax = L.xsq_wiener_resident_max_window()
    Fl, Tl = _tables(T=wmax // 2 + 2)                      # S = 2: 2 * T = wmax + 4 (or + 3) frames in one window
    for fn_args in ((L.xsq_wiener_em_iter, (p, p)), (L.xsq_wiener_em_masked_iter, (p, p, p))):
        fn, ptrs = fn_args
        ext = (None,) if fn is L.xsq_wiener_em_masked_iter else ()
        rc = fn(1, Fl.ctypes.data, Tl.ctypes.data, *ptrs, 2, 2, wmax + 2, 0, *ext, 2, 2, p, big, None)
        assert rc == XSQ_ERR_ARG and "resident" in _lib.last_error(), (rc, _lib.last_error())
    # the workspace query: 0 on bad arguments, at least the one-iteration workspace otherwise
    assert L.xsq_wiener_iter_workspace(1, F.ctypes.data, T.ctypes.data, 2, S, 250, -1, 0) == 0
    assert L.xsq_wiener_iter_workspace(1, F.ctypes.data, T.ctypes.data, 2, S, 250, 2, 5) == 0
    assert L.xsq_wiener_iter_workspace(1, F.ctypes.data, T.ctypes.data, 2, S, 250, 2, 0) >= \
        L.xsq_wiener_workspace(1, F.ctypes.data, T.ctypes.data, 2, S, 250)


def test_demixer_entry_points_refuse_a_negative_iteration_count():
    from xumx_slicq_amd import _lib
    buf = np.zeros((16, 8), dtype=np.int64)
    rc = _lib.lib.xsq_separator_schedule(18060, 18640, 1, 100000, 60000, 8, -1, 0, buf.ctypes.data, len(buf))
    assert rc == XSQ_ERR_ARG and "wiener" in _lib.last_error()


def test_schedule_does_not_depend_on_the_iteration_count():
    from xumx_slicq_amd import _lib

    def sched(nb, N, cs, max_stack, wiener, cap):
        buf = np.zeros((4096, 8), dtype=np.int64)
        n = _lib.lib.xsq_separator_schedule(18060, 18640, nb, N, cs, max_stack, wiener, cap, buf.ctypes.data, len(buf))
        assert 0 < n <= len(buf)
        return buf[:n]
    for nb, N, cs, max_stack, cap in [(1, 10_584_000, 2_621_440, 8, 0), (5, 150_000, 60000, 8, 20), (32, 2_621_440 * 3 + 100_000, 2_621_440, 8, 0)]:
        one = sched(nb, N, cs, max_stack, 1, cap)
        assert np.array_equal(sched(nb, N, cs, max_stack, 3, cap), one)
        assert one[:, 7].any() == (cap == 20 or nb == 32)       # (the split cases do share a table: the comparison sees it)


def test_niter_option_of_the_command_line():
    from xumx_slicq_amd.inference import cli_parser, parse_args
    assert parse_args(cli_parser(), []).niter is None
    assert parse_args(cli_parser(), ["--niter", "3"]).niter == 3
    assert parse_args(cli_parser(), ["--niter", "0"]).niter == 0
    for bad in (["--niter", "2", "--realtime"], ["--niter", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(cli_parser(), bad)


def test_niter_of_python_wrappers_is_checked_on_the_host():
    from xumx_slicq_amd import _lib, phase
    with pytest.raises(_lib.XsqError):
        phase._niter_method(-1, "auto")
    with pytest.raises(ValueError):
        phase._niter_method(2, "fastest")
    assert phase._niter_method(2, "resident") == (2, 2)
