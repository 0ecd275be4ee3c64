"""Fixture of the network on the logarithmic scales: tests/golden/logscale_net*.npz, from the REFERENCE's own ``Unmix`` and
``Separator.forward`` on the plans A and B of tools/make_golden_logscale.py.

Development only: the reference checkout is IMPORTED (``--reference DIR``, the directory that holds ``xumx_slicq_v2``), never
copied; the files written hold numbers and names only.  ``musdb`` is not installed here and the reference's separator does not use
it on this path: an empty stand-in module is registered under that name before the import.

Per plan (A = ``cqlog, 10, 130.0``; B = ``vqlog, 24, 40.0``, fgamma 15), on the CPU under ``no_grad``, with the seeded synthetic
weights ``seeded_state_dict(blocks, SEED)`` loaded strictly into the reference's ``Unmix`` built on the reference's own plan:

    n_<k>                                7 h + 123 samples (S = 5, ragged tail)
    sd_names_<k> (P,) str, sd_shapes_<k> (P, 5) int64     names and shapes (padded with 0) of the reference's state dict, in its order
    stems_<k>_<realtime|offline> (4, 1, 2, n) float32     ``Separator.forward`` of ``audio(n, 2)`` (the input of
                                         tests/test_logscale_cpu.py): causal mix-phase model / offline model with Wiener-EM

    python tools/make_golden_logscale_net.py --reference DIR
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# key: (scale, fbins, fmin, fgamma) -- A and B of tools/make_golden_logscale.py
PLANS = {"A": ("cqlog", 10, 130.0, 15.0), "B": ("vqlog", 24, 40.0, 15.0)}
MODELS = {"realtime": True, "offline": False}
SEED = 1234


def audio(n, rows, seed=0):
    """``tests/test_logscale_cpu.audio``: (rows, n) float32, seeded synth_audio channels, each row scaled differently."""
    from xumx_slicq_amd.synth import synth_audio
    x = torch.cat([synth_audio(n, seed=20260101 + n + seed + i)[0] for i in range((rows + 1) // 2)])[:rows]
    return (x * torch.linspace(1.0, 0.4, rows)[:, None]).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds xumx_slicq_v2/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "logscale_net.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    sys.modules.setdefault("musdb", types.ModuleType("musdb"))
    from xumx_slicq_v2.model import Unmix
    from xumx_slicq_v2.separator import Separator
    from xumx_slicq_v2.transforms import ComplexNorm, NSGTBase, make_filterbanks
    from oracle import golden
    from xumx_slicq_amd.weights import seeded_state_dict

    out = {}
    with torch.no_grad():
        for key, (scale, fbins, fmin, fgamma) in PLANS.items():
            base = NSGTBase(scale, fbins, fmin, fgamma=fgamma, device="cpu")
            nsgt, insgt = make_filterbanks(base)
            cnorm = ComplexNorm()
            n = 7 * (base.sllen // 4) + 123
            out[f"n_{key}"] = np.int64(n)
            x = audio(n, 2)[None]
            sample, _ = base.predict_input_size(1, 2, 2.0)
            sample = cnorm(sample)
            blocks = [(int(b.shape[2]), int(b.shape[4])) for b in sample]
            sd = seeded_state_dict(blocks, seed=SEED)
            for model, realtime in MODELS.items():
                unmix = Unmix(sample, realtime=realtime)
                ref_sd = unmix.state_dict()
                names = list(ref_sd)
                shapes = np.zeros((len(names), 5), dtype=np.int64)
                for i, k in enumerate(names):
                    shapes[i, :ref_sd[k].dim()] = tuple(ref_sd[k].shape)
                if model == "realtime":
                    out[f"sd_names_{key}"], out[f"sd_shapes_{key}"] = np.asarray(names), shapes
                else:
                    assert names == out[f"sd_names_{key}"].tolist() and np.array_equal(shapes, out[f"sd_shapes_{key}"])
                unmix.load_state_dict(sd, strict=True)
                sep = Separator(xumx_model=unmix, encoder=(nsgt, insgt, cnorm), sample_rate=44100.0, device="cpu", quiet=True)
                sep.freeze()
                est = sep(x).numpy().astype(np.float32)
                assert est.shape == (4, 1, 2, n) and np.isfinite(est).all(), (key, model, est.shape)
                out[f"stems_{key}_{model}"] = est
                print(key, model, "blocks", len(blocks), "longest T", max(t for _, t in blocks), "stems rms", float(np.sqrt((est ** 2).mean())))
    out["seed"] = np.int64(SEED)
    for p in golden.save(args.out, **out):
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
