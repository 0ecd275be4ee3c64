"""Fixture of the logarithmic scales: tests/golden/logscale*.npz, from the REFERENCE's own plans, transforms and slicqfinder.

Development only: the reference checkout is IMPORTED (``--reference DIR``, the directory that holds ``xumx_slicq_v2``), never
copied; the files written hold numbers only.  ``musdb`` is not installed here and the oracle does not use it: an empty
stand-in module is registered under that name before the import.

    key  plan                          L      longest band
    A    cqlog, 10, 130.0              2348   1020  (Lg 452 = 4 * 113: a prime)
    B    vqlog, 24, 40.0, fgamma 15    11652  2788  (the DC band wider than its neighbour: the flat-topped window)
    C    cqlog, 12, 20.0               13620  6416  (m = 96, 181, 343, 649, 1167, 1604)

Per plan, under ``no_grad``:

    L_<k>, tr_<k>, Lg_<k>, c_<k>         the plan's integers (bands DC .. Nyquist)
    g_<k> (sum Lg,) float32, gd_<k> (sum Lg,) float64     the analysis and dual windows, back to back
    n_<k>                                2 h + 1 samples (S = 3)
    fwd_<k>_<i> (1, 2, F, S, T, 2)       block i of NSGT_SL on synth_audio(n, seed=20260101 + n)
    inv_<k> (1, 2, n)                    INSGT_SL of those blocks
    est_<k>_<w|p>_<j> (2, n) float32     stem j of the reference's ``ideal_slicqt`` (wiener / phasemix) on the track of ``case_sources``
    sdr_<k>_<w|p> (4,) float64           its ``_fast_sdr`` per target

    python tools/make_golden_logscale.py --reference DIR
"""
import argparse
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOURCES = ("vocals", "drums", "bass", "other")
# key: (scale, fbins, fmin, fgamma)
PLANS = {"A": ("cqlog", 10, 130.0, 15.0), "B": ("vqlog", 24, 40.0, 15.0), "C": ("cqlog", 12, 20.0, 15.0)}
STRATEGIES = {"w": "wiener", "p": "phasemix"}
SEEDS, GAINS = (51, 52, 53, 54), (0.5, 0.35, 0.25, 0.4)


def case_sources(n):
    """(4, 2, n) float32: source j is gain_j * synth_audio(n, seed_j + n)[0]."""
    from xumx_slicq_amd.synth import synth_audio
    return np.stack([(np.float32(g) * synth_audio(n, seed=s + n)[0]).numpy().astype(np.float32) for s, g in zip(SEEDS, GAINS)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds xumx_slicq_v2/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "logscale.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    sys.modules.setdefault("musdb", types.ModuleType("musdb"))
    from xumx_slicq_v2 import slicqfinder as ref
    from xumx_slicq_v2.transforms import ComplexNorm, NSGTBase, make_filterbanks
    from oracle import golden
    from xumx_slicq_amd.synth import synth_audio

    out = {}
    with torch.no_grad():
        for key, (scale, fbins, fmin, fgamma) in PLANS.items():
            base = NSGTBase(scale, fbins, fmin, fgamma=fgamma, device="cpu")
            nsgt, insgt = make_filterbanks(base)
            ns = base.nsgt
            nb = ns.fbins_actual
            out[f"L_{key}"], out[f"tr_{key}"] = np.int32(base.sllen), np.int32(base.trlen)
            out[f"Lg_{key}"] = np.array([len(g) for g in ns.g[:nb]], dtype=np.int32)
            out[f"c_{key}"] = np.array([int(w[len(w) // 2]) for w in ns.wins[:nb]], dtype=np.int32)
            out[f"g_{key}"] = np.concatenate([g.numpy() for g in ns.g[:nb]]).astype(np.float32)
            out[f"gd_{key}"] = np.concatenate([g.numpy() for g in ns.gd[:nb]]).astype(np.float64)
            assert ns.gd[0].dtype == torch.float64 and ns.g[0].dtype == torch.float32
            n = 2 * (base.sllen // 4) + 1
            out[f"n_{key}"] = np.int64(n)
            C = nsgt(synth_audio(n, seed=20260101 + n))
            assert C[0].shape[3] == 3
            for i, cb in enumerate(C):
                out[f"fwd_{key}_{i}"] = cb.numpy().astype(np.float32)
            out[f"inv_{key}"] = insgt([c.clone() for c in C], n).numpy().astype(np.float32)
            src = case_sources(n)
            track = SimpleNamespace(audio=np.ascontiguousarray(src.sum(0).T),
                                    sources={name: SimpleNamespace(audio=np.ascontiguousarray(src[j].T)) for j, name in enumerate(SOURCES)})
            cnorm = ComplexNorm()
            for sk, strategy in STRATEGIES.items():
                ests = ref.ideal_slicqt(track, nsgt.forward, insgt.forward, cnorm.forward, "cpu", strategy=strategy)
                est = np.stack([ests[name].numpy() for name in SOURCES]).astype(np.float32)
                sdr = np.asarray([float(ref._fast_sdr(track, ests, target=name, device="cpu")[0]) for name in SOURCES], dtype=np.float64)
                assert est.shape == (4, 2, n) and np.isfinite(est).all() and np.isfinite(sdr).all(), (key, strategy)
                out[f"sdr_{key}_{sk}"] = sdr
                for j in range(4):
                    out[f"est_{key}_{sk}_{j}"] = est[j]
                print(key, strategy, "sdr", " ".join(f"{v:.4f}" for v in sdr))
            print(key, "L", base.sllen, "Lg", out[f"Lg_{key}"].tolist())
    out["seeds"], out["gains"] = np.asarray(SEEDS, dtype=np.int64), np.asarray(GAINS, dtype=np.float32)
    for p in golden.save(args.out, **out):
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
