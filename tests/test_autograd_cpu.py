"""CPU side of autograd through the sliCQT: the closed form of the adjoint of the FORWARD transform (dLoss/dcoef -> dLoss/dx,
``xsq_slicqt_forward_adjoint``) against float64 autograd through ``oracle.ref64.forward``, the host window the library builds its
synthesis tables from (``xsq_slicqt_forward_adjoint_window``), and the new entry points' declarations.

``forward_adjoint_closed_form`` takes a dtype: float64 is held to autograd here, float32 / complex64 is the CPU arithmetic whose
error is the E of tests/test_autograd_gpu.py.  With G the cotangent of the coefficients (real view, block list):

    V[s,j,q]   = sign_j g_j[q] / Lg_j FFT_Lg( G[s,j,:] )[q]                     sign_j = (-1)^(c_j / 2)
    k          = (c_j + sq(q)) mod L
    fr_s[k]   += V[s,j,q]                 if k <= L/2
    fr_s[L-k] += conj( V[s,j,q] )         if k >  L/2                            (the fold)
    seg_s[p]   = tw[p] irfft_L( w * fr_s )[p],  w[0] = w[L/2] = L, w[k] = L/2 otherwise    (Im of bins 0 and L/2 is dropped)
    gx[m]      = sum_s seg_s[m + 2h - 2sh],  0 <= m < n

The three switches leave one term out each: the tests hold that each of them is seen by the comparison."""
import numpy as np
import pytest
import torch

from oracle import ref64
from oracle import slicqt as O

F64, F32 = torch.float64, torch.float32
MEL = ("mel", 32, 115.5)


def mel_plan():
    return O.make_plan(*MEL)


# ---- closed form ----------------------------------------------------------------------------------------------------
def fold_entries(plan):
    """[(band, q)] whose bin (c_j + sq(q)) mod L lies above L/2: the entries the adjoint folds back, conjugated."""
    out = []
    for j in range(plan.nbands):
        k = (plan.c[j] + O._sq(int(plan.Lg[j]))) % plan.L
        out += [(j, int(q)) for q in np.nonzero(k > plan.L // 2)[0]]
    return out


def bin_weights(plan):
    w = np.full(plan.L // 2 + 1, plan.L / 2.0)
    w[0] = w[-1] = float(plan.L)
    return w


def closed_form_tables(plan):
    """Per band (fp64): g_j[q] / Lg_j * w[bin the entry lands on, after the fold] -- sign_j left out."""
    w, L = bin_weights(plan), plan.L
    out = []
    for j in range(plan.nbands):
        k = (plan.c[j] + O._sq(int(plan.Lg[j]))) % L
        out.append(plan.g[j].astype(np.float64) / float(plan.Lg[j]) * w[np.where(k > L // 2, L - k, k)])
    return out


def forward_adjoint_closed_form(plan, G_list, n, dtype=F64, fold=True, weights=True, window=True):
    """G_list: blocks (BC, F_b, S, T_b, 2) -> gx (BC, n) in ``dtype``."""
    cdt = torch.complex128 if dtype == F64 else torch.complex64
    L, h = plan.L, plan.h
    S = G_list[0].shape[-3]
    BC = G_list[0].shape[0]
    assert S == plan.nslices(n)
    fr = torch.zeros(BC, S, L // 2 + 1, dtype=cdt)
    for (j0, F, T), Gb in zip(plan.blocks, G_list):
        fc = torch.fft.fft(torch.view_as_complex(Gb.to(dtype).reshape(BC, F, S, T, 2).contiguous()))      # (BC, F, S, T)
        sq = O._sq(T)
        for f in range(F):
            j = j0 + f
            sign = 1.0 if (plan.c[j] // 2) % 2 == 0 else -1.0
            V = fc[:, f] * torch.from_numpy(plan.g[j].astype(np.float64) * (sign / T)).to(cdt)
            k = (plan.c[j] + sq) % L
            lo = k <= L // 2
            fr[:, :, torch.from_numpy(k[lo])] += V[:, :, torch.from_numpy(lo)]
            if fold and not lo.all():
                fr[:, :, torch.from_numpy(L - k[~lo])] += V[:, :, torch.from_numpy(~lo)].conj()
    w = torch.from_numpy(bin_weights(plan) if weights else np.full(L // 2 + 1, L / 2.0)).to(dtype)
    fr = fr * w
    fr[:, :, 0] = fr[:, :, 0].real.to(cdt)
    fr[:, :, -1] = fr[:, :, -1].real.to(cdt)
    seg = torch.fft.irfft(fr, n=L)
    if window:
        seg = seg * torch.from_numpy(plan.tw).to(dtype)
    y = torch.zeros(BC, (2 * S + 2) * h, dtype=dtype)
    for s in range(S):
        y[:, 2 * s * h: 2 * s * h + L] += seg[:, s]
    return y[:, 2 * h: 2 * h + n]


def random_cotangents(plan, BC, S, seed, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(BC, F, S, T, 2, generator=g, dtype=dtype) for (_, F, T) in plan.blocks]


def autograd_forward_adjoint(plan, G_list, n):
    """d <ref64.forward(x), G> / dx in float64, at a random x (the map is linear)."""
    BC = G_list[0].shape[0]
    x = torch.randn(BC, n, generator=torch.Generator().manual_seed(n), dtype=F64).requires_grad_(True)
    sum((c * g.to(F64)).sum() for c, g in zip(ref64.forward(plan, x), G_list)).backward()
    return x.grad


def forward_adjoint_window(plan):
    """The library's host window per band (list of fp64 arrays), on the oracle plan's own tables."""
    from xumx_slicq_amd import _lib
    Lg = np.ascontiguousarray(plan.Lg, dtype=np.int32)
    c = np.ascontiguousarray(plan.c, dtype=np.int32)
    g = np.ascontiguousarray(np.concatenate(plan.g), dtype=np.float32)
    out = np.full(g.shape, np.nan, dtype=np.float64)
    rc = _lib.lib.xsq_slicqt_forward_adjoint_window(plan.L, len(Lg), Lg.ctypes.data, c.ctypes.data, g.ctypes.data, out.ctypes.data)
    assert rc == 0, _lib.last_error()
    return np.split(out, np.cumsum(Lg)[:-1])


# ---- tests ----------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(oracle_plan, which, BC, n):
    """(plan, cotangents, float64 autograd), computed once per case and left unchanged."""
    key = (which, BC, n)
    if key not in _CASES:
        plan = oracle_plan if which == "bark" else mel_plan()
        G = random_cotangents(plan, BC, plan.nslices(n), seed=7 + n % 101)
        _CASES[key] = (plan, G, autograd_forward_adjoint(plan, G, n))
    return _CASES[key]


@pytest.mark.parametrize("which,BC,n", [("bark", 3, 9031), ("bark", 2, 44100), ("mel", 3, 32768)])
def test_closed_form_equals_float64_autograd_through_the_forward_transform(oracle_plan, which, BC, n):
    """Rounding of float64: measured 1.5e-14 of the largest gradient; 1e-12 allowed.  The fp32 evaluation of the same form -- the
    yardstick E of the GPU test -- is printed beside it."""
    plan, G, ref = _case(oracle_plan, which, BC, n)
    got = forward_adjoint_closed_form(plan, G, n)
    worst = float((got - ref).abs().max() / ref.abs().max())
    e32 = ref64.rel_err(forward_adjoint_closed_form(plan, [g.float() for g in G], n, dtype=F32), ref)
    print(f"forward adjoint closed form vs autograd, {which} BC {BC} n {n}: {worst:.2e} of the largest gradient; "
          f"fp32 form rel rms {float(e32[0]):.2e} max {float(e32[1]):.2e}")
    assert got.dtype == F64 and worst <= 1e-12


@pytest.mark.parametrize("which,count", [("bark", 159), ("mel", 115)])
def test_fold_counts(oracle_plan, which, count):
    plan = oracle_plan if which == "bark" else mel_plan()
    ents = fold_entries(plan)
    assert len(ents) == count
    # they come from the bands next to DC and next to Nyquist
    bands = sorted({j for j, _ in ents})
    lo = [j for j in bands if plan.c[j] < plan.L // 4]
    assert lo and lo == list(range(len(lo))) and [j for j in bands if j not in lo] == list(range(plan.nbands - (len(bands) - len(lo)), plan.nbands))


@pytest.mark.parametrize("which,BC,n", [("bark", 3, 9031), ("mel", 3, 32768)])
@pytest.mark.parametrize("term", ["fold", "weights", "window"])
def test_comparison_sees_each_term(oracle_plan, which, BC, n, term):
    """The restatement without the fold, the per-bin weights or the slice window is far from autograd: the GPU yardstick
    is not blind to any of them."""
    plan, G, ref = _case(oracle_plan, which, BC, n)
    got = forward_adjoint_closed_form(plan, G, n, **{term: False})
    worst = float((got - ref).abs().max() / ref.abs().max())
    print(f"without {term}, {which}: {worst:.2e} of the largest gradient")
    assert worst > 1e-4


@pytest.mark.parametrize("which", ["bark", "mel"])
def test_host_window_equals_the_closed_form_tables(oracle_plan, which):
    """xsq_slicqt_forward_adjoint_window = g_j[q] / Lg_j * w[bin] / L (the device's inverse slice FFT is unnormalised: the
    weights are 1 at bins 0 and L/2 and 1/2 between them), folded entries weighted by the bin they land on."""
    plan = oracle_plan if which == "bark" else mel_plan()
    got, want = forward_adjoint_window(plan), closed_form_tables(plan)
    for j, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_allclose(a * plan.L, b, rtol=1e-15, atol=0, err_msg=f"band {j}")
    k0 = (plan.c[0] + O._sq(int(plan.Lg[0]))) % plan.L
    assert got[0][k0 == 0][0] == plan.g[0][0].astype(np.float64) / plan.Lg[0]           # bin 0: weight 1
    fold = k0 > plan.L // 2                                                               # folded entries are kept, at weight 1/2
    np.testing.assert_array_equal(got[0][fold], plan.g[0][fold].astype(np.float64) / plan.Lg[0] * 0.5)
    assert (got[0][fold] != 0).any()


def test_product_plan_hands_the_same_window_to_the_library(oracle_plan):
    from xumx_slicq_amd.plan import build_plan
    p = build_plan("bark", 262, 32.9)
    np.testing.assert_array_equal(p.forward_adjoint_window(), np.concatenate(forward_adjoint_window(oracle_plan)))


def test_new_symbols_are_declared_and_exported():
    import os
    from conftest import ROOT
    from xumx_slicq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    for name in ("xsq_slicqt_forward_adjoint_workspace", "xsq_slicqt_forward_adjoint", "xsq_slicqt_forward_adjoint_window"):
        assert name + "(" in hdr, name
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED, name
    assert _lib.lib.xsq_abi_version() == 2
    from xumx_slicq_amd.transforms import SliCQEngine
    assert callable(SliCQEngine.forward_adjoint)


def test_null_arguments_return_an_error_code():
    from xumx_slicq_amd import _lib
    lib = _lib.lib
    assert lib.xsq_slicqt_forward_adjoint_workspace(None, 2, 9031) == 0
    assert lib.xsq_slicqt_forward_adjoint(None, None, 2, 9031, None, None, 0, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_slicqt_forward_adjoint_window(18060, 263, None, None, None, None) < 0 and "null" in _lib.last_error()
    Lg = np.array([16, 18], dtype=np.int32)
    c = np.array([0, 8], dtype=np.int32)
    g = np.ones(34, dtype=np.float32)
    out = np.zeros(34)
    assert lib.xsq_slicqt_forward_adjoint_window(0, 2, Lg.ctypes.data, c.ctypes.data, g.ctypes.data, out.ctypes.data) < 0
    assert "L=0" in _lib.last_error()


def test_cpu_tensors_are_refused_with_and_without_grad():
    """No device, no transform: requiring a gradient changes nothing about that."""
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.transforms import INSGT_SL, NSGT_SL, NSGTBase
    base = NSGTBase("bark", 262, 32.9, device="cpu")
    nsgt, insgt = NSGT_SL(base), INSGT_SL(base)
    for grad in (False, True):
        x = torch.zeros(1, 2, 9031, requires_grad=grad)
        with pytest.raises(_lib.XsqError, match="ROCm device only"):
            nsgt(x)
        S = base.plan.num_slices(9031)
        X = [torch.zeros(1, 2, F, S, T, 2, requires_grad=grad) for (_, F, T) in base.plan.blocks]
        with pytest.raises(_lib.XsqError, match="ROCm device only"):
            insgt(X, 9031)
