"""Fixture of the spectrogram's overlap-add: tests/golden/spectrogram_mel32.npz, from the REFERENCE's own visualization.py.

Development only: the reference checkout is IMPORTED (``--reference DIR``, the directory that holds ``xumx_slicq_v2``), never
copied; the file written holds numbers only.  ``torchaudio`` is not installed here and ``overlap_add_slicq`` does not use it: an
empty stand-in module is registered under that name before the import (matplotlib, which the module also imports, is installed).

The reference's ``NSGT_sliced.forward`` runs on a seeded stereo signal, plan ``mel, 32, 115.5``, n = 5000, exactly as
``visualization_main`` calls it (visualization.py:173-208); stored are

    x               (2, n) float32, the input
    blocks          (nblocks, 2) int64: F_b, T_b
    c_<b>           (2, F_b, S, T_b) complex64: block b after the reference's ``permute(1, 2, 0, 3)``
    ola_<b>         (2, F_b, (S + 1) T_b / 2) complex64: ``overlap_add_slicq(c_<b>)``
    flat_<b>        (2, F_b, S T_b) complex64: ``overlap_add_slicq(c_<b>, flatten=True)``

    python tools/make_golden_spectrogram.py --reference DIR
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAN = ("mel", 32, 115.5)
N = 5000
SEED = 20261021


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds xumx_slicq_v2/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spectrogram_mel32.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
    import matplotlib
    matplotlib.use("Agg")
    from xumx_slicq_v2 import visualization as ref
    from xumx_slicq_v2.nsgt import MelScale, NSGT_sliced
    from oracle import golden

    fs = 44100
    scl = MelScale(PLAN[2], 22050, PLAN[1])
    sllen, trlen = scl.suggested_sllen_trlen(fs)
    slicq = NSGT_sliced(scl, sllen, trlen, fs, real=True, multichannel=True, device="cpu")
    x = (0.1 * np.random.default_rng(SEED).standard_normal((2, N))).astype(np.float32)
    out = {"x": x}
    shapes = []
    with torch.no_grad():
        c_list = slicq.forward((torch.from_numpy(x),))
        for b, c in enumerate(c_list):
            c = c.permute(1, 2, 0, 3).contiguous()
            assert c.dim() == 4 and c.shape[0] == 2 and c.dtype == torch.complex64, (c.shape, c.dtype)
            shapes.append((c.shape[1], c.shape[3]))
            out[f"c_{b}"] = c.numpy()
            out[f"ola_{b}"] = ref.overlap_add_slicq(c).numpy()
            out[f"flat_{b}"] = ref.overlap_add_slicq(c, flatten=True).numpy()
            S, T = c.shape[2], c.shape[3]
            assert out[f"ola_{b}"].shape == (2, c.shape[1], (S + 1) * T // 2) and out[f"flat_{b}"].shape == (2, c.shape[1], S * T)
    out["blocks"] = np.asarray(shapes, dtype=np.int64)
    print("sllen", sllen, "slices", S, "blocks (F, T):", shapes)
    for p in golden.save(args.out, **out):
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
