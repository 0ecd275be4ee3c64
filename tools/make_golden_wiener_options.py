"""Fixture of the Wiener filter's option sets (softmask, residual): tests/golden/wiener_options.npz, from the REFERENCE's norbert.

Development only: the reference checkout is IMPORTED (``--reference DIR``, the directory that holds ``xumx_slicq_v2``), never
copied; the file written holds numbers only.

Inputs (seeded): the mix x (B = 2, 2 channels, F = 2 bins, 156 frames as S = 4 slices of T = 39; batch row 1 forty times
louder; the two channels correlated; frame 17 silent in both channels, frame 101 silent in channel 1) and the masks m uniform
in (0, 0.5), so that about half of the points have sum_j m_j > 1 and no residual.  Magnitudes v = m |x| in fp32.

Outputs: the semantics of the reference's ``phase.blockwise_wiener`` (phase.py:18-69) with windows of 64 frames (64 / 64 / 28)
and, per window and option set (softmask, residual, niter),

    if residual: v = norbert.contrib.residual_model(v, x, alpha=1)
    y = norbert.wiener(v, x, niter, use_softmask=softmask)

in complex64 (``Y_<case>``), and the reference's own spread (``spread_<case>``, one value per source): the relative RMS distance
of that result from the same call in complex128 WITH THE FLOAT32 EPSILONS.  norbert takes its epsilons from the dtype
(``torch.finfo(dtype).eps`` in softmask, residual_model and expectation_maximization); in float64 they are 2.2e-16 instead of
1.2e-7 and the two arithmetics then solve different problems (3e-3 to 7e-3 apart after one iteration).  The complex128 arm
therefore runs with ``torch.finfo`` answering float32's eps for every dtype (``fp32_eps`` below).

    python tools/make_golden_wiener_options.py --reference DIR
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, F, S, T, J = 2, 2, 2, 4, 39, 4
WIN = 64
CASES = ((1, 0, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 2), (0, 1, 3))        # (softmask, residual, niter)
SILENT_BOTH, SILENT_ONE = 17, 101


def case_name(softmask, residual, niter):
    return f"s{int(softmask)}r{int(residual)}k{int(niter)}"


def inputs(seed: int = 20261018):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, 1, F, S, T, 2, generator=g)
    b = torch.randn(B, C, F, S, T, 2, generator=g)
    X = (0.8 * a + 0.6 * b).float()                      # channels share `a`: correlated
    X[1] *= 40.0
    Xf = X.reshape(B, C, F, S * T, 2)
    Xf[:, :, :, SILENT_BOTH] = 0.0
    Xf[:, 1, :, SILENT_ONE] = 0.0
    m = (0.5 * torch.rand(J, B, C, F, S, T, generator=g)).float()
    mag = torch.sqrt(X[..., 0] ** 2 + X[..., 1] ** 2)
    return X.contiguous(), m.contiguous(), (m * mag).contiguous()


@contextlib.contextmanager
def fp32_eps():
    """torch.finfo(anything).eps == float32's while inside."""
    real = torch.finfo

    class _Info:
        eps = real(torch.float32).eps

    torch.finfo = lambda *a, **k: _Info
    try:
        yield
    finally:
        torch.finfo = real


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds xumx_slicq_v2/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wiener_options.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from xumx_slicq_v2 import norbert                    # the reference's vendored norbert
    from xumx_slicq_v2.norbert import contrib

    X, m, Ymag = inputs()
    N = S * T
    # phase.py:31-41: (B, C, F, S, T[, 2]) -> (B, N, F, C[, 2]) and (J, B, C, F, S, T) -> (B, N, F, C, J)
    x32 = torch.view_as_complex(X.reshape(B, C, F, N, 2).contiguous()).permute(0, 3, 2, 1).contiguous()
    v32 = Ymag.reshape(J, B, C, F, N).permute(1, 4, 3, 2, 0).contiguous()

    def run(x, v, softmask, residual, niter):
        Jo = J + int(residual)
        y = torch.zeros(B, N, F, C, Jo, dtype=x.dtype)
        for p in range(0, N, WIN):
            vw, xw = v[:, p:p + WIN], x[:, p:p + WIN]
            if residual:
                vw = contrib.residual_model(vw, xw, 1)
            y[:, p:p + WIN] = norbert.wiener(vw, xw, niter, use_softmask=bool(softmask))
        return y

    out = {}
    for softmask, residual, niter in CASES:
        name = case_name(softmask, residual, niter)
        y32 = run(x32, v32, softmask, residual, niter)
        with fp32_eps():
            y64 = run(x32.to(torch.complex128), v32.double(), softmask, residual, niter)
        assert bool(torch.isfinite(torch.view_as_real(y32)).all()) and bool(torch.isfinite(torch.view_as_real(y64)).all())
        d = (y32.to(torch.complex128) - y64).abs().pow(2).mean((0, 1, 2, 3)).sqrt() / y64.abs().pow(2).mean((0, 1, 2, 3)).sqrt()
        Jo = J + residual
        out[f"Y_{name}"] = torch.view_as_real(y32).permute(4, 0, 3, 2, 1, 5).contiguous().reshape(Jo, B, C, F, S, T, 2).numpy()
        out[f"spread_{name}"] = d.numpy()
        print(name, "spread per source", " ".join(f"{float(e):.2e}" for e in d))
    share = float((m.sum(0) > 1).float().mean())
    print("share of points with sum of masks > 1:", share)
    np.savez_compressed(args.out, X=X.numpy(), masks=m.numpy(), Ymag=Ymag.numpy(), win_len=np.int32(WIN),
                        cases=np.asarray(CASES, dtype=np.int32), **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
