"""Generate tests/golden/plans3_<name>.npz by running the REFERENCE itself (imported from /root/reference, never copied) on
plans other than its two shipped ones.  Development container only: the reference does not travel to the GPU box; the
fixtures do.

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_plans

Per plan: the reference's sllen, trlen, band table and block shapes; the forward coefficients of the S = 3 clip
(n = 4h - 77 samples of ``synth_audio``, B = 1), whole or as checksums; the waveform decoded from them; the waveform
decoded from BLOCK 0 ALONE (every other block zero), which is where a band that reaches across DC lives; and for plan T
the waveform decoded from seeded normal coefficients, which are no transform's output, so the reference's mirrored
synthesis (nsgt/nsigtf.py:57-99, quirk A12) is pinned on input that is not Hermitian-consistent.  Block lists are cloned
before decoding (the reference decoder overwrites its input, quirk A1).  The cases are those of
tests/test_ref64_plans_cpu.py; M (``mel, 64, 115.5``) is the plan the GPU module runs beside W.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import golden
from oracle.make_golden import checksums
from xumx_slicq_amd.synth import synth_audio

OUT = os.path.join(ROOT, "tests", "golden")
PLANS = {"T": ("bark", 28, 32.9), "K": ("bark", 56, 32.9), "W": ("bark", 400, 300.0), "M": ("mel", 64, 115.5)}
FULL_BLOCKS = {"W": 9}             # blocks stored whole (the others as checksums); absent: all
RANDOM_SEED = 2803                 # the seeded normal coefficients of plan T


def random_coefs(shapes, seed=RANDOM_SEED):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) for s in shapes]


def main():
    torch.set_num_threads(8)
    from xumx_slicq_v2.transforms import NSGTBase, make_filterbanks
    os.makedirs(OUT, exist_ok=True)
    for name, cfg in PLANS.items():
        base = NSGTBase(*cfg, fs=44100.0, device="cpu")
        enc, dec = make_filterbanks(base, 44100.0)
        ns = base.nsgt
        nb = ns.fbins_actual
        n = base.sllen - 77
        x = synth_audio(n, seed=20260101 + n)
        with torch.no_grad():
            C = enc(x)
            y = dec([c.clone() for c in C], n)
            y0 = dec([c.clone() if i == 0 else torch.zeros_like(c) for i, c in enumerate(C)], n)
        d = dict(L=base.sllen, tr=base.trlen, nbands=nb, n=n, S=C[0].shape[3],
                 Lg=np.array([len(g) for g in ns.g[:nb]], dtype=np.int32),
                 c=np.array([int(w[len(w) // 2]) for w in ns.wins[:nb]], dtype=np.int32),
                 blocks=np.array([[b.shape[2], b.shape[4]] for b in C], dtype=np.int32),
                 fwd_sums=np.stack([checksums(cb) for cb in C]), inv=y.numpy(), inv_block0=y0.numpy())
        for i, cb in enumerate(C[:FULL_BLOCKS.get(name, len(C))]):
            d[f"fwd_{i}"] = cb.numpy()
        if name == "T":
            R = random_coefs([c.shape for c in C])
            with torch.no_grad():
                d["inv_random"] = dec([r.clone() for r in R], n).numpy()
            d["random_sums"] = np.stack([checksums(r) for r in R])
            d["random_seed"] = RANDOM_SEED
        for p in golden.save(os.path.join(OUT, f"plans3_{name}.npz"), **d):
            print(os.path.basename(p), os.path.getsize(p))


if __name__ == "__main__":
    main()
