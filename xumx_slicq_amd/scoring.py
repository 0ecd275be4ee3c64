"""Scores of a separation computed where the waveforms are: framewise and global SDR on the device (csrc/score.hip).

The reference scores a track with ``museval.eval_mus_track`` on the host (xumx_slicq_v2/evaluation.py:16-44) and has
``_fast_sdr`` for the whole-track ratio (xumx_slicq_v2/slicqfinder.py:20-40).  BSSEval v4's SDR of source IMAGES needs none of
its 512-tap projection filters: the three error terms sum to ``estimate - reference``, so a frame's SDR is
``10 log10(sum s^2 / sum (s_hat - s)^2)`` over the frame's samples and both channels.  That is a streaming reduction over
the estimates ``Separator.forward`` left in HBM and the targets ``data.DeviceDataset`` keeps there; only the finalised
numbers (a few hundred doubles) go to the host.

The metric, named ``"framewise-sdr"`` for what it is (DESIGN.md section 7.2 has the full definition):
  * a track of N samples has ``max(1, N // W)`` frames ``[k W, (k + 1) W)``, W = ``window`` samples (default
    ``round(sample_rate)``); hop = window; a tail shorter than W is dropped; N < W is one frame over the whole track;
  * frame value ``10 log10(num / den)`` with ``num = sum s^2``, ``den = sum (s_hat - s)^2`` formed in fp64 from the fp32 samples;
    ``den == 0`` gives +inf; a silent frame gives NaN;
  * ``silent="any"``: a frame is NaN for every target when any target's reference or estimate has zero energy in it;
    ``silent="own"``: when the target's own reference has;
  * ``sdr_median``: nanmedian of a target's frames; ``sdr_global``: ``10 log10((sum s^2 + 1e-10) / (sum (s_hat - s)^2 + 1e-10))``
    over the whole track, the dropped tail included (= ``evaluation.global_sdr`` = the reference's ``_fast_sdr``).
The framing (one-second windows, hop = window, the tail dropped) and the silence rule follow ``museval.metrics.bss_eval`` AS
REMEMBERED: museval is not a dependency of this project and was not available, so the rule could not be checked against the package.  ISR, SIR
and SAR need the projection filters and are not computed.

Targets are matched to estimates by NAME, never by position: ``Separator.sources`` is bass, vocals, other, drums while
``DeviceDataset.sources`` is vocals, drums, bass, other.  A fifth, residual stem of the estimates has no target and is ignored.

There is no CPU path: CPU tensors raise ``XsqError``.  Every launch goes to the caller's current stream; a scorer belongs to one
stream at a time.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

METRIC = "framewise-sdr"
SILENT_MODES = {"any": 0, "own": 1}
_SOURCES = ("bass", "vocals", "other", "drums")            # Separator.sources (separator.py imports the whole model stack)


def max_frames() -> int:
    """The most frames a track may have: the median is a sort in LDS (xsq_score_max_frames)."""
    return int(_lib.lib.xsq_score_max_frames())


def window_samples(window: Optional[int], sample_rate: float = 44100.0, hop: Optional[int] = None) -> int:
    """W in samples: ``window``, or one second.  ``hop``: only the window itself; overlapping or gapped frames are not built."""
    W = int(round(float(sample_rate))) if window is None else int(window)
    if W < 1:
        raise ValueError(f"window {window}: at least one sample")
    if hop is not None and int(hop) != W:
        raise ValueError(f"hop {hop} != window {W}: framewise-sdr frames do not overlap (hop = window), as museval's default")
    return W


def frame_layout(length: int, window: int) -> Tuple[int, int, int]:
    """(frames, samples per frame, samples of the dropped tail) of a track of ``length`` samples."""
    N, W = int(length), int(window)
    if N < 1 or W < 1:
        raise ValueError(f"length {length}, window {window}: both at least 1")
    if N < W:
        return 1, N, 0
    return N // W, W, N - (N // W) * W


def target_permutation(target_order: Sequence[str], estimate_order: Sequence[str] = _SOURCES) -> Tuple[int, ...]:
    """perm[i] = the stem of the estimates that has the name of target i."""
    target_order, estimate_order = tuple(target_order), tuple(estimate_order)
    if len(target_order) != 4 or len(set(target_order)) != 4:
        raise ValueError(f"target_order names four different targets; got {target_order}")
    unknown = [t for t in target_order if t not in estimate_order]
    if unknown:
        raise ValueError(f"unknown target(s) {unknown}: the estimates are {estimate_order}")
    return tuple(estimate_order.index(t) for t in target_order)


def check_shapes(estimates, targets, nb_samples: Optional[int] = None) -> None:
    """ValueError unless estimates is (4 | 5, B, 2, n) and targets (4, B, 2, n), n >= 1 (B = ``nb_samples`` when given)."""
    ok = isinstance(estimates, Tensor) and isinstance(targets, Tensor) and estimates.dim() == 4 and targets.dim() == 4
    if ok:
        B = targets.shape[1] if nb_samples is None else nb_samples
        ok = estimates.shape[0] in (4, 5) and targets.shape[0] == 4 and tuple(estimates.shape[1:]) == (B, 2, targets.shape[3]) \
            and tuple(targets.shape[1:3]) == (B, 2) and targets.shape[3] >= 1 and B >= 1
    if not ok:
        got = [tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__ for t in (estimates, targets)]
        raise ValueError(f"expected estimates (4 | 5, {'B' if nb_samples is None else nb_samples}, 2, n) and targets "
                         f"(4, {'B' if nb_samples is None else nb_samples}, 2, n); got {got[0]} / {got[1]}")


def _rows(t: Tensor, B: int) -> Tuple[Tensor, int]:
    """(tensor, row stride): rows (stem, b, channel) a fixed number of floats apart and unit stride along time -- a view
    ``full[..., a:b]`` of a contiguous tensor is taken as it is; anything else is copied."""
    n = t.shape[3]
    rs = t.stride(2)
    ok = t.stride(3) == 1 and rs >= n and (B == 1 or t.stride(1) == 2 * rs) and t.stride(0) == 2 * B * rs
    if not ok:
        t = t.contiguous()
        rs = n
    return t, rs


class TrackScorer:
    """Scores ``nb_samples`` tracks of ``length`` samples piece by piece.

    ``add(estimates, targets)`` takes consecutive pieces: estimates (4 | 5, nb_samples, 2, n) in ``estimate_order``, targets
    (4, nb_samples, 2, n) in ``target_order``, fp32 on the device.  Pieces may start and end anywhere inside a frame.
    ``result()`` finalises on the device and brings the numbers to the host."""

    def __init__(self, nb_samples: int, length: int, window: Optional[int] = None, silent: str = "any", sample_rate: float = 44100.0,
                 target_order: Sequence[str] = _SOURCES, device="cuda", hop: Optional[int] = None,
                 estimate_order: Sequence[str] = _SOURCES):
        if silent not in SILENT_MODES:
            raise ValueError(f"silent {silent!r}: 'any' (a frame is dropped when any target's reference or estimate is silent in it) "
                             "or 'own' (when the target's own reference is)")
        self.window = window_samples(window, sample_rate, hop)
        self.silent, self.nb_samples, self.length = silent, int(nb_samples), int(length)
        if self.nb_samples < 1:
            raise ValueError(f"nb_samples {nb_samples}: at least one row")
        self.frames, self.frame_len, self.tail = frame_layout(self.length, self.window)
        self.target_order, self.estimate_order = tuple(target_order), tuple(estimate_order)
        self.perm = target_permutation(self.target_order, self.estimate_order)
        self._perm = (C.c_int * 4)(*self.perm)
        tb, wb = C.c_size_t(0), C.c_size_t(0)
        _lib.call("xsq_score_workspace", self.nb_samples, self.length, self.window, C.byref(tb), C.byref(wb))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.XsqError("scores are computed on a ROCm device only; there is no CPU fallback")
        self._table = torch.empty(tb.value // 8, dtype=torch.float64, device=self.device)
        self._ws = torch.empty(wb.value, dtype=torch.uint8, device=self.device)
        self.position = 0                  # where the next piece starts by default
        self._covered = self._scored = 0   # pieces never overlap: the next one starts at or behind _covered

    def add(self, estimates: Tensor, targets: Tensor, offset: Optional[int] = None) -> "TrackScorer":
        B = self.nb_samples
        check_shapes(estimates, targets, B)
        if estimates.device.type != "cuda" or targets.device != estimates.device or estimates.device != self._table.device:
            raise _lib.XsqError(f"the scoring kernels run on a ROCm device only ({self._table.device} here); there is no CPU fallback "
                                f"(got {estimates.device} / {targets.device})")
        if estimates.dtype != torch.float32 or targets.dtype != torch.float32:
            raise ValueError(f"expected fp32 waveforms; got {estimates.dtype} / {targets.dtype}")
        if max(self.perm) >= estimates.shape[0]:
            raise ValueError(f"the estimates have {estimates.shape[0]} stems; targets {self.target_order} need stem {max(self.perm)}")
        n = int(targets.shape[3])
        off = self.position if offset is None else int(offset)
        if off < 0 or off + n > self.length:
            raise ValueError(f"piece [{off}, {off + n}) is out of range: the track has {self.length} samples")
        if off < self._covered:
            raise ValueError(f"piece [{off}, {off + n}) overlaps what is already scored (everything before sample {self._covered})")
        est, es = _rows(estimates.detach(), B)
        tgt, ts = _rows(targets.detach(), B)
        with torch.cuda.device(self._table.device):
            if self._scored == 0:
                self._table.zero_()
            _lib.call("xsq_score_accumulate", est.data_ptr(), tgt.data_ptr(), C.cast(self._perm, C.c_void_p), B, n, es, ts, off,
                      self.length, self.window, self._table.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream_ptr())
        self.position = self._covered = off + n
        self._scored += n
        return self

    def result(self) -> Dict:
        if self._scored != self.length:
            raise ValueError(f"{self._scored} of the track's {self.length} samples were added: add the rest first")
        B, F = self.nb_samples, self.frames
        with torch.cuda.device(self._table.device):
            frames = torch.empty(4, B, F, dtype=torch.float64, device=self._table.device)
            scores = torch.empty(4, B, 2, dtype=torch.float64, device=self._table.device)
            _lib.call("xsq_score_finalise", self._table.data_ptr(), B, F, SILENT_MODES[self.silent], frames.data_ptr(), scores.data_ptr(),
                      _lib.stream_ptr())
            frames, scores = frames.cpu().numpy(), scores.cpu().numpy()        # the only device-to-host traffic
        return {"metric": METRIC, "window": self.window, "silent": self.silent,
                "targets": {name: {"sdr_median": [float(v) for v in scores[i, :, 0]], "sdr_global": [float(v) for v in scores[i, :, 1]],
                                   "frames": frames[i]} for i, name in enumerate(self.target_order)}}


def score(estimates: Tensor, targets: Tensor, window: Optional[int] = None, silent: str = "any", sample_rate: float = 44100.0,
          target_order: Sequence[str] = _SOURCES, hop: Optional[int] = None, estimate_order: Sequence[str] = _SOURCES) -> Dict:
    """One shot: whole tracks, estimates (4 | 5, B, 2, N) against targets (4, B, 2, N).  See ``TrackScorer``."""
    check_shapes(estimates, targets)
    if estimates.device.type != "cuda":
        raise _lib.XsqError(f"the scoring kernels run on a ROCm device only; there is no CPU fallback (got {estimates.device})")
    scorer = TrackScorer(targets.shape[1], targets.shape[3], window=window, silent=silent, sample_rate=sample_rate,
                         target_order=target_order, device=estimates.device, hop=hop, estimate_order=estimate_order)
    return scorer.add(estimates, targets).result()


def to_jsonable(result):
    """A result with arrays as lists and the values JSON has no word for spelled out: NaN -> null, +-inf -> "inf" / "-inf"."""
    if isinstance(result, dict):
        return {k: to_jsonable(v) for k, v in result.items()}
    if isinstance(result, np.ndarray):
        return to_jsonable(result.tolist())
    if isinstance(result, (list, tuple)):
        return [to_jsonable(v) for v in result]
    if isinstance(result, (float, np.floating)):
        v = float(result)
        return None if v != v else ("inf" if v > 0 else "-inf") if v in (float("inf"), float("-inf")) else v
    return result
