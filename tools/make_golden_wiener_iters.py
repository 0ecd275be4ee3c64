"""Fixture of the many-iteration Wiener filter: tests/golden/wiener_iters.npz, from the REFERENCE's norbert.

Development only: the reference checkout is IMPORTED (``--reference DIR``, the directory that holds ``xumx_slicq_v2``), never
copied; the file written holds numbers only.

Inputs (seeded): the mix x (B = 2, 2 channels, F = 2 bins, 612 frames as S = 4 slices of T = 153; batch row 1 forty times
louder; the two channels correlated) and magnitudes v = m |x| with m uniform in (0, 1).  Outputs: the semantics of the
reference's ``phase.blockwise_wiener`` (phase.py:18-69) with ``iterations`` = 2 and 3 in place of its literal 1 and windows of
250 frames (250 / 250 / 112): per window ``norbert.wiener(v, x, k, use_softmask=False)`` (norbert/__init__.py:153-260) on
the window's slice of (frames, bins, channels[, sources]) with the batch folded as the reference folds it.

    python tools/make_golden_wiener_iters.py --reference DIR
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, F, S, T, J = 2, 2, 2, 4, 153, 4
WIN = 250
ITERS = (2, 3)


def inputs(seed: int = 20260702):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, 1, F, S, T, 2, generator=g)
    b = torch.randn(B, C, F, S, T, 2, generator=g)
    X = (0.8 * a + 0.6 * b).float()                      # channels share `a`: correlated
    X[1] *= 40.0
    m = torch.rand(J, B, C, F, S, T, generator=g).float()
    mag = torch.sqrt(X[..., 0] ** 2 + X[..., 1] ** 2)
    return X.contiguous(), (m * mag).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds xumx_slicq_v2/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wiener_iters.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from xumx_slicq_v2 import norbert                    # the reference's vendored norbert

    X, Ymag = inputs()
    N = S * T
    # phase.py:31-41: (B, C, F, S, T[, 2]) -> (B, N, F, C[, 2]) and (J, B, C, F, S, T) -> (B, N, F, C, J)
    x = torch.view_as_complex(X.reshape(B, C, F, N, 2).contiguous()).permute(0, 3, 2, 1).contiguous()
    v = Ymag.reshape(J, B, C, F, N).permute(1, 4, 3, 2, 0).contiguous()
    out = {}
    for k in ITERS:
        y = torch.zeros(B, N, F, C, J, dtype=torch.complex64)
        for p in range(0, N, WIN):
            y[:, p:p + WIN] = norbert.wiener(v[:, p:p + WIN], x[:, p:p + WIN], k, False)
        y = torch.view_as_real(y).permute(4, 0, 3, 2, 1, 5).contiguous().reshape(J, B, C, F, S, T, 2)
        out[f"Y_k{k}"] = y.numpy()
    np.savez_compressed(args.out, X=X.numpy(), Ymag=Ymag.numpy(), win_len=np.int32(WIN), iters=np.asarray(ITERS, dtype=np.int32), **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
