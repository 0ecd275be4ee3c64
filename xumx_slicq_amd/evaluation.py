"""Mirror of /root/reference/xumx_slicq_v2/evaluation.py:16-44 (``separate_and_evaluate``): track audio ->
``preprocess_audio`` -> ``separator(audio)`` -> ``Separator.to_dict`` -> per-target scores.

The reference scores with ``museval.eval_mus_track`` on a ``musdb.MultiTrack``; neither package (nor MUSDB18-HQ,
nor trained weights) exists offline.  This mirror takes any track object with the three attributes the reference
reads (``audio`` (T, C) array, ``rate``, ``targets`` {name: object with ``.audio`` (T, C)}), runs the same
separation call, and scores with museval when it is importable; otherwise it reports the global
signal-to-distortion ratio 10 log10(|s|^2 / |s - s_hat|^2) per target (the "new SDR" of the Music Demixing
Challenge -- NOT BSSEval v4; the result says which one it is).  The separation half is the accelerated hot path;
the scoring half is CPU bookkeeping.

``evaluate_dataset`` and the command line (``python -m xumx_slicq_amd.evaluation``) are the loop over a test set
(evaluation.py:45-118) for stems that are on the device already (``data.DeviceDataset``): estimates and targets are scored
where they lie (``scoring.TrackScorer``: framewise and global SDR) and only the finalised numbers reach the host.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .audio import preprocess_audio
from .separator import Separator


def global_sdr(reference: np.ndarray, estimate: np.ndarray, eps: float = 1e-10) -> float:
    """10 log10(sum s^2 / sum (s - s_hat)^2) over all samples and channels of one target."""
    ref = np.asarray(reference, dtype=np.float64)
    est = np.asarray(estimate, dtype=np.float64)
    n = min(ref.shape[0], est.shape[0])
    ref, est = ref[:n], est[:n]
    return float(10.0 * np.log10((np.sum(ref * ref) + eps) / (np.sum((ref - est) ** 2) + eps)))


def separate_and_evaluate(separator: Separator, track, device: Union[str, torch.device] = "cuda") -> Dict:
    """evaluation.py:16-44.  Returns {"metric": "museval-bsseval-v4" | "global-sdr", "scores": ...,
    "estimates": {target: (T, C) float32 array}}."""
    audio = torch.as_tensor(np.asarray(track.audio), dtype=torch.float32, device=device)
    audio = preprocess_audio(audio, track.rate, float(separator.sample_rate))
    estimates = separator.to_dict(separator(audio))
    estimates = {k: v[0].detach().cpu().numpy().T for k, v in estimates.items()}      # (T, C), as museval wants them
    try:
        import museval
    except ImportError:                 # only the import: an error INSIDE museval must not turn into the other metric
        museval = None
    if museval is not None:
        return {"metric": "museval-bsseval-v4", "scores": museval.eval_mus_track(track, estimates), "estimates": estimates}
    scores = {name: global_sdr(np.asarray(track.targets[name].audio), est)
              for name, est in estimates.items() if name in getattr(track, "targets", {})}
    return {"metric": "global-sdr", "scores": scores, "estimates": estimates}


# ---- scores that never leave the device (scoring.py, csrc/score.hip) ------------------------------------------------------
def _track_indices(dataset, tracks) -> List[int]:
    if tracks is None:
        return list(range(len(dataset)))
    out = []
    for t in tracks:
        if isinstance(t, str):
            if t not in dataset.names:
                raise ValueError(f"no track {t!r} in the dataset (it has {dataset.names})")
            out.append(dataset.names.index(t))
        else:
            if not 0 <= int(t) < len(dataset):
                raise ValueError(f"track {t} of a dataset of {len(dataset)}")
            out.append(int(t))
    return out


def _nanmedian(values) -> float:
    v = np.asarray(values, dtype=np.float64)
    return float(np.median(v[~np.isnan(v)])) if (~np.isnan(v)).any() else float("nan")


def aggregate_scores(per_track: Dict[str, Dict]) -> Dict:
    """Per target over the tracks' results: the median of ``sdr_median`` (tracks in which the target is silent throughout
    carry NaN and are left out, as a nanmedian), and the mean and median of ``sdr_global``."""
    out = {}
    for res in per_track.values():
        for name, sc in res["targets"].items():
            o = out.setdefault(name, {"m": [], "g": []})
            o["m"] += list(sc["sdr_median"])
            o["g"] += list(sc["sdr_global"])
    return {name: {"sdr_median": _nanmedian(o["m"]), "sdr_global_mean": float(np.mean(o["g"])), "sdr_global_median": float(np.median(o["g"]))}
            for name, o in out.items()}


def evaluate_dataset(separator: Separator, dataset, tracks: Optional[Sequence] = None, window: Optional[int] = None,
                     silent: str = "any") -> Dict:
    """The evaluation loop of evaluation.py:45-118 over a ``data.DeviceDataset``, scored on the device: per track, every piece
    of ``dataset.pieces(i, separator.chunk_size)`` goes through ``separator`` and estimate and target into a
    ``scoring.TrackScorer`` -- neither leaves the device.  ``tracks``: indices or names (default: all).  ``window``: samples
    per frame (default one second).  The targets of a piece come in ``dataset.targets`` order and the estimates in
    ``separator.sources`` order; they are matched by name.

    Returns {"metric": "framewise-sdr", "window", "silent", "tracks": {name: TrackScorer.result()}, "aggregate": {target:
    {"sdr_median", "sdr_global_mean", "sdr_global_median"}}} (``aggregate_scores``)."""
    from .scoring import METRIC, TrackScorer, window_samples
    W = window_samples(window, float(separator.sample_rate))
    per_track = {}
    for i in _track_indices(dataset, tracks):
        scorer = TrackScorer(1, int(dataset.lengths[i]), window=W, silent=silent, target_order=dataset.targets,
                             estimate_order=separator.sources, device=dataset.device)
        for x, y in dataset.pieces(i, separator.chunk_size):
            scorer.add(separator(x), y)
        per_track[dataset.names[i]] = scorer.result()
    return {"metric": METRIC, "window": W, "silent": silent, "tracks": per_track, "aggregate": aggregate_scores(per_track)}


def cli_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m xumx_slicq_amd.evaluation",
                                description="framewise and global SDR of xumx-sliCQ-V2 over a directory of tracks, scored on the MI355X")
    p.add_argument("--root", type=str, required=True, help="<root>/<track>/{vocals,drums,bass,other}.wav, the MUSDB18-HQ layout")
    p.add_argument("--tracks", type=str, default=None, metavar="NAME,...", help="the track directories to score (default: all, sorted)")
    p.add_argument("--model-path", type=str, default=None,
                   help="directory with xumx_slicq_v2.json/.pth; omit for seeded synthetic weights")
    p.add_argument("--realtime", action="store_true")
    p.add_argument("--niter", type=int, default=None, metavar="N",
                   help="EM iterations of the Wiener post-filter of the offline model (default 1; 0 = mix-phase); not with --realtime")
    p.add_argument("--softmask", action="store_true", help="start the Wiener post-filter from the ratio mask; not with --realtime")
    p.add_argument("--window-seconds", type=float, default=1.0, metavar="SECONDS", help="frame length (hop = window; default 1.0)")
    p.add_argument("--silent", choices=("any", "own"), default="any",
                   help="a frame is dropped when ANY target's reference or estimate is silent in it (default), or the target's OWN reference")
    p.add_argument("--storage", choices=("fp32", "pcm16"), default="fp32", help="how the stems are kept on the device (pcm16: 16-bit files only)")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--out", type=str, required=True, help="directory for <track>.json and aggregate.json")
    p.add_argument("--long-bands", action="store_true",
                   help="accept a model trained on the cqlog or vqlog scale: its bands above 320 samples run on the FFT band engine")
    p.add_argument("--fgamma", type=float, default=15.0, metavar="HZ",
                   help="offset of the vqlog band centres where the model's JSON names none (default 15.0)")
    return p


def parse_args(p: argparse.ArgumentParser, argv=None):
    """``p.parse_args`` plus the checks between options.  Host only."""
    args = p.parse_args(argv)
    if args.niter is not None:
        if args.niter < 0:
            p.error(f"--niter {args.niter}: the iteration count is >= 0")
        if args.realtime:
            p.error("--niter counts the EM iterations of the offline model's Wiener filter; --realtime is mix-phase and has none")
    if args.softmask and args.realtime:
        p.error("--softmask is an option of the offline model's Wiener filter; --realtime is mix-phase and has none")
    if not (0 < args.window_seconds < float("inf")):
        p.error(f"--window-seconds {args.window_seconds}: a positive number of seconds")
    args.tracks = [t for t in args.tracks.split(",") if t] if args.tracks else None
    return args


def evaluation_main(argv=None) -> Dict:
    """One track at a time on the device: its stems are uploaded, demixed, scored and dropped."""
    import json
    from .data import DeviceDataset
    from .scoring import METRIC, to_jsonable
    from .separator import seeded_separator
    p = cli_parser()
    args = parse_args(p, argv)
    if args.model_path:
        separator = Separator.load(model_path=args.model_path, runtime_backend="hip-rocm", realtime=args.realtime, device=args.device,
                                   niter=args.niter, softmask=args.softmask or None, long_bands=args.long_bands, fgamma=args.fgamma)
    else:
        separator = seeded_separator(realtime=args.realtime, device=args.device, niter=args.niter, softmask=args.softmask or None,
                                     long_bands=args.long_bands, fgamma=args.fgamma)
    names = args.tracks
    if names is None:
        names = sorted(d for d in os.listdir(args.root)
                       if all(os.path.isfile(os.path.join(args.root, d, s + ".wav")) for s in DeviceDataset.sources))
    if not names:
        p.error(f"no track directory with {DeviceDataset.sources} .wav files under {args.root}")
    W = max(1, int(round(args.window_seconds * float(separator.sample_rate))))
    os.makedirs(args.out, exist_ok=True)
    per_track = {}
    for name in names:
        ds = DeviceDataset.from_directory(args.root, names=[name], storage=args.storage, device=args.device)
        res = evaluate_dataset(separator, ds, window=W, silent=args.silent)["tracks"][name]
        per_track[name] = res
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(to_jsonable(dict(res, track=name)), f, indent=1)
        print(f"{name}: " + "  ".join(f"{t} {sc['sdr_median'][0]:.3f} dB" for t, sc in res["targets"].items()))
    agg = {"metric": METRIC, "window": W, "silent": args.silent, "tracks": list(names), "aggregate": aggregate_scores(per_track)}
    with open(os.path.join(args.out, "aggregate.json"), "w") as f:
        json.dump(to_jsonable(agg), f, indent=1)
    print("median over tracks: " + "  ".join(f"{t} {a['sdr_median']:.3f} dB" for t, a in agg["aggregate"].items()))
    return agg


if __name__ == "__main__":
    evaluation_main()
