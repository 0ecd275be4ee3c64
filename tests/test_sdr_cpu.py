"""CPU side of the SDR loss term: the adjoint window a' of the inverse sliCQT (``xsq_slicqt_adjoint_window``, host arithmetic)
against float64 autograd through ``oracle.ref64.inverse``, the float64 SDR formula against its own definition, and the new
entry points' declarations.  The closed forms here (``adjoint_closed_form``, ``inverse_dtype``, ``sdr_criterion``) take a dtype:
float64 is the reference, float32 / complex64 the CPU arithmetic whose error is the E of tests/test_sdr_gpu.py.

The SD-SDR formula is auraloss 0.4's ``SDSDRLoss`` (zero_mean, eps = 1e-8, mean reduction) as stated in DESIGN.md section 7;
auraloss is not a dependency of this project and the formula is the contract."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import ref64
from oracle import slicqt as O

F64, F32 = torch.float64, torch.float32
EPS = 1e-8
COMBOS = [c for r in (1, 2, 3) for c in itertools.combinations(range(4), r)]        # the reference's order (loss.py:17-32)


# ---- closed forms ---------------------------------------------------------------------------------------------------
def adjoint_window(plan):
    """a' per band (list of fp64 arrays) from the library's host function, on the oracle plan's own tables."""
    from xumx_slicq_amd import _lib
    Lg = np.ascontiguousarray(plan.Lg, dtype=np.int32)
    c = np.ascontiguousarray(plan.c, dtype=np.int32)
    gd = np.ascontiguousarray(np.concatenate(plan.gd), dtype=np.float64)
    out = np.full_like(gd, np.nan)
    rc = _lib.lib.xsq_slicqt_adjoint_window(plan.L, len(Lg), Lg.ctypes.data, c.ctypes.data, gd.ctypes.data, out.ctypes.data)
    assert rc == 0, _lib.last_error()
    return np.split(out, np.cumsum(Lg)[:-1])


def adjoint_closed_form(plan, aw, gy, S, dtype=F64):
    """gy (BC, n) -> list over blocks of (BC, F_b, S, T_b, 2): gcoef[s,j,:] = sign_j IFFT_Lg( a'_j[q] V_s[c_j + sq(q)] ),
    V_s = rfft_L( gypad[(2s-2)h : (2s+2)h] ), no slice window."""
    L, h = plan.L, plan.h
    BC, n = gy.shape
    pad = torch.zeros(BC, (2 * S + 2) * h, dtype=dtype)
    pad[:, 2 * h: 2 * h + n] = gy.to(dtype)
    V = torch.fft.rfft(pad.unfold(-1, L, 2 * h)[:, :S])                                  # (BC, S, L/2 + 1)
    out = []
    for (j0, F, T) in plan.blocks:
        k = plan.c[j0:j0 + F, None] + O._sq(T)[None, :]
        ok = (k >= 0) & (k <= L // 2)
        a = np.stack(aw[j0:j0 + F])
        assert not a[~ok].any()                                                         # zero wherever the bin does not exist
        sign = torch.from_numpy(np.where((plan.c[j0:j0 + F] // 2) % 2 == 0, 1.0, -1.0)).to(dtype)
        cb = torch.fft.ifft(V[:, :, torch.from_numpy(np.where(ok, k, 0))] * torch.from_numpy(a).to(dtype)) * sign[None, None, :, None]
        out.append(torch.view_as_real(cb.permute(0, 2, 1, 3).contiguous()))
    return out


def inverse_dtype(plan, X_list, length, dtype=F64):
    """``ref64.inverse`` with the arithmetic in ``dtype`` (ref64.inverse casts to float64)."""
    cdt = torch.complex128 if dtype == F64 else torch.complex64
    L, h = plan.L, plan.h
    lead = X_list[0].shape[:-4]
    S = X_list[0].shape[-3]
    BC = int(np.prod(lead)) if len(lead) else 1
    fr = torch.zeros(BC, S, L // 2 + 1, dtype=cdt)
    for (j0, F, T), Xb in zip(plan.blocks, X_list):
        fc = torch.fft.fft(torch.view_as_complex(Xb.to(dtype).reshape(BC, F, S, T, 2).contiguous()))
        sq = O._sq(T)
        for f in range(F):
            j = j0 + f
            sign = 1.0 if (plan.c[j] // 2) % 2 == 0 else -1.0
            w = torch.from_numpy(plan.gd[j] * (T * sign)).to(cdt)
            k = plan.c[j] + sq
            keep = (k >= 0) & (k <= L // 2)
            fr[:, :, torch.from_numpy(k[keep])] += (fc[:, f] * w)[:, :, torch.from_numpy(keep)]
    seg = torch.fft.irfft(fr, n=L)
    y = torch.zeros(BC, (2 * S + 2) * h, dtype=dtype)
    for s in range(S):
        y[:, 2 * s * h: 2 * s * h + L] += seg[:, s]
    return y[:, 2 * h: 2 * h + length].reshape(*lead, length)


def sdsdr_rows(p, t):
    """SDSDRLoss per row, before the mean: p, t (..., n) in their own dtype."""
    p = p - p.mean(-1, keepdim=True)
    t = t - t.mean(-1, keepdim=True)
    alpha = (p * t).sum(-1) / ((t * t).sum(-1) + EPS)
    res = p - t                                                                          # NOT p - alpha * t
    return -10.0 * torch.log10(((alpha[..., None] * t) ** 2).sum(-1) / ((res * res).sum(-1) + EPS) + EPS)


def sdr_criterion(pred, target, dtype=F64):
    """SDRLossCriterion (loss.py:5-34) on (4, B, 2, n) waveforms -> (scalar, (14, B, 2) row losses)."""
    p, t = pred.to(dtype), target.to(dtype)
    rows = torch.stack([sdsdr_rows(sum(p[i] for i in c), sum(t[i] for i in c)) for c in COMBOS])
    return rows.mean(), rows


def random_blocks(plan, BC, S, seed, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(BC, F, S, T, 2, generator=g, dtype=dtype) for (_, F, T) in plan.blocks]


def autograd_adjoint(plan, BC, n, seed):
    """(gy, [d <y, gy> / d coef per block]) in float64 through ref64.inverse, at random coefficients (the map is linear)."""
    S = plan.nslices(n)
    X = [x.requires_grad_(True) for x in random_blocks(plan, BC, S, seed)]
    gy = torch.randn(BC, n, generator=torch.Generator().manual_seed(seed + 1), dtype=F64)
    (ref64.inverse(plan, X, n) * gy).sum().backward()
    return gy, [x.grad for x in X], S


# ---- tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,n", [("bark", 9031), ("mel", 1513), ("mel", 32768)])
def test_adjoint_window_closed_form_equals_float64_autograd_through_the_inverse(oracle_plan, which, n):
    """Rounding of float64: measured 3.8e-16 relative max on Bark-262 at n = 9031; 1e-12 allowed."""
    plan = oracle_plan if which == "bark" else O.make_plan("mel", 32, 115.5)
    aw = adjoint_window(plan)
    gy, ref, S = autograd_adjoint(plan, 2, n, seed=5)
    got = adjoint_closed_form(plan, aw, gy, S)
    worst = 0.0
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape
        worst = max(worst, float((g - r).abs().max() / r.abs().max()))
    print(f"adjoint closed form vs autograd, {which} n={n}: worst relative max error over {len(ref)} blocks {worst:.2e}")
    assert worst <= 1e-12


def test_adjoint_window_is_not_symmetric_and_vanishes_on_mirrored_bins(oracle_plan):
    plan = oracle_plan
    aw = adjoint_window(plan)
    L = plan.L
    for j in (0, plan.nbands - 1):                      # DC and Nyquist: the half of the window past the end of the spectrum
        k = plan.c[j] + O._sq(int(plan.Lg[j]))
        assert (aw[j][(k < 0) | (k > L // 2)] == 0).all() and (aw[j][(k >= 0) & (k <= L // 2)] != 0).any()
    j = plan.nbands // 2
    n = int(plan.Lg[j])
    np.testing.assert_allclose(aw[j], 2.0 * n * n * plan.gd[j] / L, rtol=1e-15)
    # gd is symmetric in q only to fp32 rounding of the windows it is made from (1e-7 relative), and the DC / Nyquist
    # bands' a' not at all: nothing downstream may pair q with Lg - q
    assert not np.array_equal(aw[j][1:], aw[j][1:][::-1])
    assert not np.allclose(aw[0][1:], aw[0][1:][::-1], rtol=1e-3)


def test_product_plan_hands_the_same_window_to_the_library(oracle_plan):
    from xumx_slicq_amd.plan import build_plan
    p = build_plan("bark", 262, 32.9)
    np.testing.assert_array_equal(p.adjoint_window(), np.concatenate(adjoint_window(oracle_plan)))


def test_sdr_formula_silent_target_is_finite_with_zero_gradient():
    """A self-check of this file's float64 formula (the reference of tests/test_sdr_gpu.py), not of the library: it passes with or
    without the feature.  What the kernels do on the same input is held on the GPU."""
    g = torch.Generator().manual_seed(3)
    p = torch.randn(4, 1, 2, 500, generator=g, dtype=F64).requires_grad_(True)
    t = torch.randn(4, 1, 2, 500, generator=g, dtype=F64)
    t[2, 0, 1] = 0.0
    loss, rows = sdr_criterion(p, t)
    assert torch.isfinite(rows).all() and abs(float(rows[2, 0, 1].detach()) - 80.0) < 1e-9
    rows[2, 0, 1].backward()
    assert float(p.grad.abs().max()) == 0.0


def test_new_symbols_are_declared_and_exported():
    import os
    from conftest import ROOT
    from xumx_slicq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    for name in ("xsq_sdr_loss_workspace", "xsq_sdr_loss_forward", "xsq_sdr_loss_backward", "xsq_slicqt_adjoint_window",
                 "xsq_slicqt_inverse_adjoint_workspace", "xsq_slicqt_inverse_adjoint", "xsq_train_workspace_sdr",
                 "xsq_train_step_sdr", "xsq_train_loss_sdr"):
        assert name + "(" in hdr, name
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED, name
    assert _lib.lib.xsq_abi_version() == 2
    from xumx_slicq_amd.loss import SDRLossCriterion, validation_step          # noqa: F401
    import inspect
    from xumx_slicq_amd.training import Trainer
    assert inspect.signature(Trainer.__init__).parameters["sdr_mcoef"].default == -1.0
    assert inspect.signature(validation_step).parameters["sdr_mcoef"].default == -1.0


def test_null_arguments_return_an_error_code():
    from xumx_slicq_amd import _lib
    lib = _lib.lib
    assert lib.xsq_sdr_loss_workspace(0, 100) == 0 and lib.xsq_sdr_loss_workspace(1, 0) == 0
    assert lib.xsq_sdr_loss_workspace(1, 9031) > 0
    assert lib.xsq_sdr_loss_forward(None, None, 1, 100, None, None, 0, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_sdr_loss_backward(None, None, 1, 100, 1.0, None, None, None, 0, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_slicqt_adjoint_window(18060, 263, None, None, None, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_slicqt_inverse_adjoint_workspace(None, 2, 3, 0) == 0
    assert lib.xsq_slicqt_inverse_adjoint(None, None, 2, 3, 9031, None, 0, None, 0, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_train_workspace_sdr(None, None, 1, 3, 1, 9031) == 0
    assert lib.xsq_train_step_sdr(None, None, None, None, None, 9031, 1.0, 1, 3, 1, 1e-3, 1e-5, 0, None, None, 0, None) < 0
    assert "null" in _lib.last_error()
    out = (C.c_double * 3)()
    assert lib.xsq_train_loss_sdr(None, 0, out) < 0
