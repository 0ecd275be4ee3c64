"""The ideal-mask oracle and the sliCQT parameter search of xumx_slicq_v2/slicqfinder.py on the HIP library.

``ideal_slicqt`` answers "what could a perfect network reach with this filterbank": the true stems are transformed, their
magnitudes borrow the phase of the mix (``strategy="phasemix"``) or go through one block-wise Wiener-EM iteration
(``"wiener"``), and the result is inverted (slicqfinder.py:43-117).  It is ONE native call, ``xsq_ideal_separate``: the
forward transform of the four stems stacked as rows is already the estimates' arena, the filter reads that arena in place
(``xsq_wiener_em_sources`` / ``xsq_phasemix_sources``, csrc/wiener.hip) and the inverse transform follows -- no mix arena,
no magnitudes.  ``TrackEvaluator`` scores the estimates on the device (``scoring.TrackScorer``) over the tracks of a
``data.DeviceDataset`` and ``optimize_many`` draws (scale, bins, fmin) and keeps the best, as the reference does.

Departures from the reference, all deliberate:
  * a track is transformed in pieces of ``piece`` samples (default: the Separator's chunk, 2,621,440), not whole; a ``piece``
    of the track's own length is the reference's behaviour where the arena fits one launch;
  * the draws are ONE table made up front from ``numpy.random.default_rng(seed)`` (``draw_params``): a search is reproducible
    anywhere (the reference seeds ``random`` but draws the bins from the unseeded ``numpy.random``);
  * the logarithmic scales ``cqlog`` and ``vqlog`` are drawn only with ``long_bands`` (``--long-bands``), which runs their upper
    bands on the FFT band engine; without it they are refused by name, and with it a draw whose longest band exceeds
    ``plan.long_band_max()`` is refused and counted like any other;
  * a plan with a band across DC is refused by ``build_plan`` (the library leaves out that band's mirrored synthesis term);
    the oracle then returns four ``-inf`` like a too-long slice, and every refusal is counted and named in the result.

There is no CPU path: CPU tensors raise ``XsqError``.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

STRATEGIES = {"wiener": 0, "phasemix": 1}              # XSQ_IDEAL_WIENER, XSQ_IDEAL_PHASEMIX (include/xumx_slicq_hip.h)
ORACLE_TARGETS = ("bass", "drums", "vocals", "other")  # the order of TrackEvaluator.oracle's tuple (slicqfinder.py:179-201)
SCALES = ("bark", "mel")                               # what plan.build_plan builds
LONG_SCALES = ("bark", "mel", "cqlog", "vqlog")        # ... with long_bands=True
LONG_DEFAULT_SCALES = ("bark", "mel", "cqlog")         # the reference's default draw (slicqfinder.py: --fscale)
DEFAULT_PIECE = 2621440                                # Separator.chunk_size
NEG_INF4 = (float("-inf"),) * 4
NO_REASON = "the oracle returned four -inf without a reason"


def ideal_slicqt(sources: Tensor, base, strategy: str = "wiener", wiener_win_len: int = 5000, niter: int = 1) -> Tensor:
    """sources (4, B, 2, n) fp32 on a ROCm device, ``base`` an ``NSGTBase`` -> estimates (4, B, 2, n), stem j of item b
    where source j of item b was.  Every batch item is a track of its own (its own Wiener window maximum).
    ``wiener_win_len`` = 0: one window over all frames of a block, as the reference's ``blockwise_wiener`` takes it.
    ``niter``: only 1 -- the mix exists only on chip, a further EM iteration needs it in memory."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy {strategy!r} not in {sorted(STRATEGIES)}")
    if int(niter) != 1:
        raise _lib.XsqError(f"ideal_slicqt runs one EM iteration (got niter={niter}): a further one needs the mix in memory; "
                            "write the estimates and use phase.wiener_em_arena")
    if not isinstance(sources, Tensor) or sources.dim() != 4 or sources.shape[0] != 4 or sources.shape[2] != 2 or sources.shape[3] < 1:
        got = tuple(sources.shape) if isinstance(sources, Tensor) else type(sources).__name__
        raise ValueError(f"expected the four sources as (4, B, 2, n); got {got}")
    if sources.device.type != "cuda":
        raise _lib.XsqError(f"ideal_slicqt runs on a ROCm device only (got '{sources.device}'); there is no CPU fallback")
    win = int(wiener_win_len) if wiener_win_len else 0
    if win < 0:
        raise ValueError(f"wiener_win_len {wiener_win_len}: a frame count, or 0 for one window over all frames")
    src = sources.detach().to(torch.float32).contiguous()
    _, B, _, n = src.shape
    eng = base.nsgt
    d = eng.demixer(src.device)
    with torch.cuda.device(src.device):
        ws = eng.workspace(src.device, _lib.workspace_bytes("xsq_ideal_workspace", d, B, n, STRATEGIES[strategy], win))
        out = torch.empty_like(src)
        _lib.call("xsq_ideal_separate", d, src.data_ptr(), B, n, STRATEGIES[strategy], win, out.data_ptr(), ws.data_ptr(), ws.numel(),
                  _lib.stream_ptr())
    return out


def filter_sources_arena(table, Sc: Tensor, Y: Tensor, B: int, S: int, strategy: str = "wiener", win_len: int = 5000, batch_group: int = 1) -> Tensor:
    """The filter alone on the arena level (``xsq_wiener_em_sources`` / ``xsq_phasemix_sources``): Sc = the coefficients of the
    four sources, an arena of 8B complex channels (what ``SliCQEngine.forward`` returns for a (4, B, 2, n) input), Y an arena of
    the same size that takes the estimates; ``Y is Sc`` runs in place.  ``table``: the plan's ``arena.BlockTable``."""
    from .phase import _tables, _workspace
    if Sc.device.type != "cuda" or Y.device != Sc.device:
        raise _lib.XsqError(f"the oracle's filter runs on a ROCm device only (got '{Sc.device}' / '{Y.device}'); there is no CPU fallback")
    need = table.numel(8 * B, S)
    for t in (Sc, Y):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != need:
            raise ValueError(f"expected a contiguous fp32 arena of {need} floats (8 * {B} channels, {S} slices); got {t.dtype} x {t.numel()}")
    F, T = _tables(table)
    geometry = (len(table), F.ctypes.data, T.ctypes.data)
    with torch.cuda.device(Sc.device):
        if strategy == "phasemix":
            _lib.call("xsq_phasemix_sources", *geometry, Sc.data_ptr(), Y.data_ptr(), B, S, _lib.stream_ptr())
            return Y
        if strategy != "wiener":
            raise ValueError(f"strategy {strategy!r} not in {sorted(STRATEGIES)}")
        ws = _workspace(Sc.device, _lib.workspace_bytes("xsq_wiener_sources_workspace", *geometry, B, S, int(win_len), why="bad arguments"))
        _lib.call("xsq_wiener_em_sources", *geometry, Sc.data_ptr(), Y.data_ptr(), B, S, int(win_len), int(batch_group), ws.data_ptr(),
                  ws.numel(), _lib.stream_ptr())
    return Y


class TrackEvaluator:
    """slicqfinder.py:120-201 over a ``data.DeviceDataset``.  ``oracle(scale, fmin, bins)`` -> the SDRs of bass, drums,
    vocals, other: per target the mean over ``tracks`` (indices or names; default all) of the whole-track ``sdr_global``.
    ``dc_twins``: score the plans with bands across DC too, decoded with the reference's mirrored synthesis
    (``plan.build_plan``); by default such a draw is refused.  ``long_bands``: score ``cqlog`` and ``vqlog`` too, their bands above
    320 on the FFT band engine; by default those scales are refused."""

    def __init__(self, dataset, max_sllen: int = 44100, piece: Optional[int] = None, tracks: Optional[Sequence] = None,
                 strategy: str = "wiener", wiener_win_len: int = 5000, dc_twins: bool = False, long_bands: bool = False):
        from .evaluation import _track_indices
        if strategy not in STRATEGIES:
            raise ValueError(f"strategy {strategy!r} not in {sorted(STRATEGIES)}")
        self.dataset, self.max_sllen = dataset, int(max_sllen)
        self.piece = DEFAULT_PIECE if piece is None else int(piece)
        if self.piece < 1:
            raise ValueError(f"piece {piece}: at least one sample")
        self.tracks = _track_indices(dataset, tracks)
        self.strategy, self.wiener_win_len = strategy, int(wiener_win_len)
        self.dc_twins = bool(dc_twins)
        self.long_bands = bool(long_bands)
        self.refusals: List[Dict] = []                 # every draw that was not scored, with the reason

    def _refuse(self, scale, fmin, bins, reason) -> Tuple[float, float, float, float]:
        self.refusals.append({"scale": scale, "bins": int(bins), "fmin": float(fmin), "reason": reason})
        return NEG_INF4

    def oracle(self, scale: str = "bark", fmin: float = 32.9, bins: int = 262) -> Tuple[float, float, float, float]:
        from .scoring import TrackScorer
        from .transforms import NSGTBase
        bins = int(bins)
        try:
            base = NSGTBase(scale, bins, float(fmin), device=self.dataset.device, dc_twins=self.dc_twins, long_bands=self.long_bands)
        except ValueError as e:                        # an unknown scale, a band across DC, a band too long: plan.build_plan says which
            return self._refuse(scale, fmin, bins, f"plan refused: {e}")
        if base.sllen > self.max_sllen:                # slicqfinder.py:137: "skip too big transforms"
            return self._refuse(scale, fmin, bins, f"sllen {base.sllen} > max_sllen {self.max_sllen}")
        ds = self.dataset
        per_target = {t: [] for t in ds.targets}
        try:
            for i in self.tracks:
                scorer = TrackScorer(1, int(ds.lengths[i]), target_order=ds.targets, estimate_order=ds.targets, device=ds.device)
                for _, y in ds.pieces(i, self.piece):
                    scorer.add(ideal_slicqt(y, base, self.strategy, self.wiener_win_len), y)
                res = scorer.result()["targets"]
                for t in ds.targets:
                    per_target[t].append(res[t]["sdr_global"][0])
        finally:
            base.nsgt.close()                          # the plan's device tables go before the next draw builds its own
        return tuple(float(np.mean(per_target[t])) for t in ORACLE_TARGETS)


def draw_params(seed: int, n_iter: int, scales: Sequence[str], bins: Tuple[int, int], fmins: Tuple[float, float, float]) -> List[Tuple[str, int, float]]:
    """The search's draws as one table, a pure function of its arguments: from ``numpy.random.default_rng(seed)`` three
    arrays of ``n_iter`` are drawn in this order -- the scale index, the bins ``integers(bins[0], bins[1])`` (upper end
    excluded, numpy.random.randint's rule, slicqfinder.py:245) and the index into ``numpy.arange(*fmins)`` (:239, :246)."""
    scales = list(scales)
    grid = np.arange(*[float(v) for v in fmins])
    if n_iter < 0 or not scales or int(bins[0]) >= int(bins[1]) or grid.size == 0:
        raise ValueError(f"n_iter {n_iter}, scales {scales}, bins {tuple(bins)}, fmins {tuple(fmins)}: nothing to draw from")
    rng = np.random.default_rng(int(seed))
    si = rng.integers(0, len(scales), size=n_iter)
    bi = rng.integers(int(bins[0]), int(bins[1]), size=n_iter)
    fi = rng.integers(0, grid.size, size=n_iter)
    return [(scales[int(s)], int(b), float(grid[int(f)])) for s, b, f in zip(si, bi, fi)]


def _is_reroll(scores) -> bool:
    return all(s == float("-inf") for s in scores)


def _reason(refusals: Optional[List], before: int) -> str:
    """Why the oracle refused its last draw: what it appended to ``refusals`` during that call."""
    new = refusals[before:] if refusals is not None else []
    return "; ".join(str(r.get("reason", r)) if isinstance(r, dict) else str(r) for r in new) or NO_REASON


def optimize_many(f: Callable, params: Dict, n_iter: int, per_target: bool = False, seed: int = 42, out: Optional[str] = None,
                  refusals: Optional[List] = None, dc_twins: Optional[bool] = None, long_bands: Optional[bool] = None) -> Dict:
    """slicqfinder.py:225-354: ``n_iter`` scored rounds; a draw whose oracle value is four ``-inf`` is rerolled (the next
    row of the table is taken in its place) and counted.  ``params``: {"scales", "bins": (lo, hi), "fmin": (lo, hi, step)}.
    The table holds ``8 * n_iter + 8`` draws; a search that exhausts it stops short and says so (``"exhausted"``).
    ``refusals``: the list ``f`` appends its reasons to (``TrackEvaluator.refusals`` for ``TrackEvaluator.oracle``); whatever it
    gained during a refused call becomes that draw's reason, and a draw refused without one says so (``NO_REASON``).
    Returns -- and, with ``out``, writes as JSON -- the best score and parameters (per target with ``per_target``), every
    scored round, and under ``"refusals"`` every rerolled draw with its reason (``"rerolled"`` counts them).  ``dc_twins``, ``long_bands``
    (when given): the evaluator's flags, recorded in the result under those names."""
    table = draw_params(seed, 8 * int(n_iter) + 8, params["scales"], params["bins"], params["fmin"])
    names = ORACLE_TARGETS if per_target else ("total",)
    best = {t: {"sdr": float("-inf"), "params": None} for t in names}
    rounds, rerolls, k = [], [], 0
    while len(rounds) < n_iter and k < len(table):
        scale, bins, fmin = table[k]
        k += 1
        before = len(refusals) if refusals is not None else 0
        scores = tuple(float(s) for s in f(scale=scale, fmin=fmin, bins=bins))
        if _is_reroll(scores):
            rerolls.append({"scale": scale, "bins": bins, "fmin": fmin, "reason": _reason(refusals, before)})
            print(f"({scale}, {bins}, {fmin}) not scored ({rerolls[-1]['reason'][:80]}): drawing again")
            continue
        rounds.append({"scale": scale, "bins": bins, "fmin": fmin, "sdr": dict(zip(ORACLE_TARGETS, scores)), "total": sum(scores) / 4})
        cur = dict(zip(ORACLE_TARGETS, scores)) if per_target else {"total": sum(scores) / 4}
        for t in names:
            if cur[t] > best[t]["sdr"]:
                best[t] = {"sdr": cur[t], "params": (scale, bins, fmin)}
                print(f"round {len(rounds)}: best {t} so far {cur[t]:.3f} dB at {(scale, bins, fmin)}")
    for t in names:
        print(f"best {t}: {best[t]['sdr']:.3f} dB at {best[t]['params']}")
    result = {"seed": int(seed), "n_iter": int(n_iter), "per_target": bool(per_target), "params": {k_: list(v) for k_, v in params.items()},
              "best": best, "rounds": rounds, "rerolled": len(rerolls), "refusals": rerolls,
              "exhausted": len(rounds) < n_iter}
    if dc_twins is not None:
        result["dc_twins"] = bool(dc_twins)
    if long_bands is not None:
        result["long_bands"] = bool(long_bands)
    _write(result, out)
    return result


def evaluate_single(f: Callable, params: Dict, out: Optional[str] = None, refusals: Optional[List] = None,
                    dc_twins: Optional[bool] = None, long_bands: Optional[bool] = None) -> Dict:
    """slicqfinder.py:204-222: one (scale, bins, fmin).  ``refusals``, ``dc_twins``: as in ``optimize_many``; a refused parameter set
    is named with its reason under ``"refusals"``."""
    before = len(refusals) if refusals is not None else 0
    scores = tuple(float(s) for s in f(scale=params["scale"], fmin=params["fmin"], bins=params["bins"]))
    print("  ".join(f"{t} {v:.2f} dB" for t, v in zip(ORACLE_TARGETS, scores)) + f"  mean {sum(scores) / 4:.2f} dB")
    result = {"params": dict(params), "sdr": dict(zip(ORACLE_TARGETS, scores)), "total": sum(scores) / 4,
              "refusals": [dict(params, reason=_reason(refusals, before))] if _is_reroll(scores) else []}
    if dc_twins is not None:
        result["dc_twins"] = bool(dc_twins)
    if long_bands is not None:
        result["long_bands"] = bool(long_bands)
    _write(result, out)
    return result


def _write(result: Dict, out: Optional[str]) -> None:
    if out:
        from .scoring import to_jsonable
        d = os.path.dirname(os.path.abspath(out))
        os.makedirs(d, exist_ok=True)
        with open(out, "w") as fh:
            json.dump(to_jsonable(result), fh, indent=1)


def cli_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m xumx_slicq_amd.slicqfinder", description="ideal-mask SDR of sliCQT parameter sets over validation tracks, scored on the MI355X")
    p.add_argument("--fbins", type=str, default="10,300", metavar="LO,HI", help="bins are drawn from [LO, HI); with --single: the one bin count")
    p.add_argument("--fmins", type=str, default="10,130,0.1", metavar="LO,HI,STEP", help="fmin is drawn from the grid LO, LO + STEP, ... below HI (Hz); with --single: the one fmin")
    p.add_argument("--n-iter", type=int, default=60, help="scored rounds of the search")
    p.add_argument("--fscale", type=str, default=None, metavar="NAME,...",
                   help="frequency scales to draw from: bark, mel (the default), and with --long-bands cqlog, vqlog (default then: bark,mel,cqlog)")
    p.add_argument("--oracle-strategy", type=str, default="wiener", choices=sorted(STRATEGIES), help="one Wiener-EM iteration (default) or the mix phase on the true magnitudes")
    p.add_argument("--random-seed", type=int, default=42, help="seed of the draw table")
    p.add_argument("--max-sllen", type=int, default=44100, help="a plan with a longer slice is not scored and the round is drawn again")
    p.add_argument("--single", action="store_true", help="score the one parameter set --fscale / --fbins / --fmins name; no search")
    p.add_argument("--per-target", action="store_true", help="keep the best parameter set of each target, not of their mean")
    p.add_argument("--dc-twins", action="store_true", help="score plans with bands across DC too (the reference's mirrored synthesis on the device); by default they are drawn again")
    p.add_argument("--long-bands", action="store_true", help="open the logarithmic scales cqlog and vqlog: their bands above 320 run on the FFT band engine")
    p.add_argument("--root", type=str, required=True, help="<root>/<track>/{vocals,drums,bass,other}.wav, the MUSDB18-HQ layout")
    p.add_argument("--valid", type=str, default=None, metavar="NAME,...", help="the validation track directories (default: all, sorted)")
    p.add_argument("--storage", choices=("fp32", "pcm16"), default="fp32", help="how the stems are kept on the device (pcm16: 16-bit files only)")
    p.add_argument("--piece", type=int, default=DEFAULT_PIECE, metavar="SAMPLES", help="samples transformed at a time (default: the Separator's chunk)")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--out", type=str, default="slicqfinder.json", help="the result, as JSON")
    return p


def parse_args(p: argparse.ArgumentParser, argv=None):
    """``p.parse_args`` plus the checks between options.  Host only."""
    args = p.parse_args(argv)
    if args.fscale is None:
        args.fscale = ",".join(LONG_DEFAULT_SCALES if args.long_bands else SCALES)
    args.scales = [s for s in args.fscale.split(",") if s]
    allowed = LONG_SCALES if args.long_bands else SCALES
    for s in args.scales:
        if s in LONG_SCALES and s not in allowed:
            p.error(f"--fscale {s}: the logarithmic scales need --long-bands (their upper bands run on the FFT band engine); without it: {SCALES}")
        if s not in allowed:
            p.error(f"--fscale {s}: not in {allowed}")
    if not args.scales:
        p.error("--fscale: at least one scale")
    try:
        if args.single:
            if len(args.scales) != 1:
                p.error("--single takes one --fscale")
            args.params = {"scale": args.scales[0], "bins": int(args.fbins), "fmin": float(args.fmins)}
        else:
            bins = tuple(int(x) for x in args.fbins.split(","))
            fmins = tuple(float(x) for x in args.fmins.split(","))
            if len(bins) != 2 or len(fmins) != 3:
                raise ValueError("ranges")
            args.params = {"scales": args.scales, "bins": bins, "fmin": fmins}
    except ValueError:
        p.error("--fbins LO,HI and --fmins LO,HI,STEP (with --single: one value each)")
    if args.n_iter < 1 or args.piece < 1:
        p.error("--n-iter and --piece are at least 1")
    args.valid = [t for t in args.valid.split(",") if t] if args.valid else None
    return args


def slicqfinder_main(argv=None) -> Dict:
    from .data import DeviceDataset
    p = cli_parser()
    args = parse_args(p, argv)
    ds = DeviceDataset.from_directory(args.root, names=args.valid, storage=args.storage, device=args.device)
    ev = TrackEvaluator(ds, args.max_sllen, piece=args.piece, strategy=args.oracle_strategy, dc_twins=args.dc_twins, long_bands=args.long_bands)
    if args.single:
        return evaluate_single(ev.oracle, args.params, out=args.out, refusals=ev.refusals, dc_twins=ev.dc_twins, long_bands=ev.long_bands)
    print(f"searching scales {args.params['scales']}, bins {args.params['bins']}, fmin {args.params['fmin']}; sllen at most {args.max_sllen}")
    return optimize_many(ev.oracle, args.params, args.n_iter, args.per_target, seed=args.random_seed, out=args.out, refusals=ev.refusals,
                         dc_twins=ev.dc_twins, long_bands=ev.long_bands)


if __name__ == "__main__":
    slicqfinder_main()
