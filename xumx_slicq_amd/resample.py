"""Sample-rate conversion of the front end: ``torchaudio.transforms.Resample(rate, model_rate,
resampling_method="sinc_interpolation")`` of data.py:148-156 (preprocess_audio) without torchaudio.

torchaudio builds a polyphase filter ``K`` of ``n`` phases x ``2*width + o`` taps (Hann window, ``lowpass_filter_width``
zero crossings, cut-off ``rolloff`` x the lower Nyquist rate; ``o`` / ``n`` the rates divided by their gcd) and applies
it as ``conv1d(x_pad, K, stride=o)``.  Outside about ``12*o/base`` taps around each phase's centre every entry of ``K``
is exactly 0 in fp32 (the window and the sinc underflow together), so this module keeps only each phase's non-zero run:
an ``n x span`` table and the index of its first tap per phase (``resample_table``).  The conv itself is the HIP kernel
``xsq_resample`` (csrc/resample.hip): no CPU path.

Two details follow torchaudio 2.x as written and could not be checked against it offline: the phase offsets ``-p/n`` are
computed in float32 before the taps' float64 arithmetic, and the output length is ``ceil(float32(n * L / o))``.
"""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib

# Largest compact table (n x span entries) built: 64 MiB of fp32.  Rate pairs whose reduced new rate n is this large
# (e.g. 44100 -> 44099 has n = 44099 phases, ~13 taps each) stay far below it.
MAX_TABLE_ENTRIES = 1 << 24

METHODS = ("sinc_interpolation", "sinc_interp_hann")


@dataclass(frozen=True)
class ResampleTable:
    """The host side of one (orig, new) pair: the compacted filter (numpy) and its geometry."""
    orig: int                 # o = orig_freq / gcd
    new: int                  # n = new_freq / gcd
    width: int                # torchaudio's padding: ceil(lowpass_filter_width * o / base)
    span: int                 # taps kept per phase (the longest non-zero run)
    table: np.ndarray         # float32 (n, span): K[p, first_tap[p] + i]
    first_tap: np.ndarray     # int32 (n,): index of table[p, 0] among K's 2*width + o taps

    def output_length(self, length: int) -> int:
        return output_length(length, self.orig, self.new)


def _rates(orig_freq, new_freq) -> Tuple[int, int]:
    out = []
    for f in (orig_freq, new_freq):
        v = float(f)
        if not math.isfinite(v) or v != int(v) or v <= 0:
            raise ValueError(f"sample rates must be positive integers, got {f!r}")
        out.append(int(v))
    return out[0], out[1]


def reduced_rates(orig_freq, new_freq) -> Tuple[int, int]:
    """(o, n): the rates divided by their gcd."""
    a, b = _rates(orig_freq, new_freq)
    g = math.gcd(a, b)
    return a // g, b // g


def output_length(length: int, o: int, n: int) -> int:
    """torchaudio's target length, ceil of a float32 (n * L / o), within the conv's (L // o + 1) * n outputs."""
    want = int(np.ceil(np.float32(n * int(length) / o)))
    return min(want, (int(length) // o + 1) * n)


def filter_geometry(o: int, n: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[float, int]:
    """(base, width) of torchaudio's kernel for the reduced rates."""
    base = min(o, n) * rolloff
    return base, int(math.ceil(lowpass_filter_width * o / base))


def filter_taps(p: np.ndarray, k: np.ndarray, o: int, n: int, lowpass_filter_width: int = 6,
                rolloff: float = 0.99) -> np.ndarray:
    """K[p, k] in float32 for phases p and tap indices k (0 .. 2*width + o - 1, broadcast together); taps outside
    that range are 0."""
    base, width = filter_geometry(o, n, lowpass_filter_width, rolloff)
    p = np.asarray(p, dtype=np.int64)
    k = np.asarray(k, dtype=np.int64)
    phase = (-p.astype(np.float32) / np.float32(n)).astype(np.float64)      # -p/n: float32, then promoted
    t = phase + (k - width).astype(np.float64) / o
    t = np.clip(t * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    taps = (sinc * (window * (base / o))).astype(np.float32)
    return np.where((k >= 0) & (k < 2 * width + o), taps, np.float32(0))


def resample_table(orig_freq, new_freq, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> ResampleTable:
    """The compacted filter of (orig_freq -> new_freq), never forming K's full n x (2*width + o) table."""
    o, n = reduced_rates(orig_freq, new_freq)
    if lowpass_filter_width <= 0 or not (0 < rolloff <= 1):
        raise ValueError(f"lowpass_filter_width {lowpass_filter_width} / rolloff {rolloff}")
    base, width = filter_geometry(o, n, lowpass_filter_width, rolloff)
    # candidate window per phase: every non-zero tap has |t * base| < lowpass_filter_width, i.e. lies within
    # half = lowpass_filter_width * o / base taps of the phase's centre k = width + o * p / n
    half = lowpass_filter_width * o / base
    cand = int(math.ceil(2 * half)) + 8
    if n * cand > MAX_TABLE_ENTRIES:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz needs a filter table of {n} phases x ~{cand} taps, "
                         f"more than the {MAX_TABLE_ENTRIES} entries this resampler builds")
    p = np.arange(n, dtype=np.int64)
    k0 = np.floor(width + o * p / n - half).astype(np.int64) - 3
    k = k0[:, None] + np.arange(cand, dtype=np.int64)[None, :]
    taps = filter_taps(p[:, None], k, o, n, lowpass_filter_width, rolloff)
    nz = taps != 0
    if not nz.any(axis=1).all():
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz: a phase without taps")
    first = nz.argmax(axis=1)
    last = cand - 1 - nz[:, ::-1].argmax(axis=1)
    # the window must hold every non-zero tap with room for the longest run after each phase's first tap
    assert first.min() > 0 and last.max() < cand - 1, (orig_freq, new_freq)
    span = int((last - first).max()) + 1
    assert int(first.max()) + span <= cand, (orig_freq, new_freq)
    table = np.ascontiguousarray(np.take_along_axis(taps, first[:, None] + np.arange(span)[None, :], axis=1))
    return ResampleTable(o, n, width, span, table, (k0 + first).astype(np.int32))


_CACHE: Dict[tuple, tuple] = {}
_LOCK = threading.Lock()


def _device_table(o: int, n: int, lowpass_filter_width: int, rolloff: float, device: torch.device):
    """(ResampleTable, table tensor, first_tap tensor) on `device`, built and uploaded once per key (like the plan)."""
    key = (o, n, int(lowpass_filter_width), float(rolloff), device)
    hit = _CACHE.get(key)
    if hit is None:
        with _LOCK:
            hit = _CACHE.get(key)
            if hit is None:
                tab = resample_table(o, n, lowpass_filter_width, rolloff)
                hit = (tab, torch.from_numpy(tab.table).to(device), torch.from_numpy(tab.first_tap).to(device))
                _CACHE[key] = hit
    return hit


def _rows(x: torch.Tensor):
    """(rows view, row stride) of (..., L) with unit stride along L, as a view whenever the leading dims flatten."""
    L = x.shape[-1]
    if x.dim() == 1:
        x = x[None]
    if x.stride(-1) != 1:
        x = x.contiguous()
    rows = x.reshape(-1, L)               # a view when the leading dimensions flatten with one stride, a copy otherwise
    return rows, (rows.stride(0) if rows.shape[0] > 1 else L)


def resample(waveform: torch.Tensor, orig_freq, new_freq, lowpass_filter_width: int = 6,
             rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.functional.resample (Hann window) of (..., L) float32 on the GPU: (..., L') on the same device,
    L' = ceil(float32(new * L / orig)) with the rates divided by their gcd.  Equal rates return `waveform` itself.
    Runs on the current stream; once the table of a (rates, device) exists it allocates only the output and never
    synchronises (capturable into a graph)."""
    o, n = reduced_rates(orig_freq, new_freq)
    if o == n:
        return waveform
    if waveform.device.type != "cuda":
        raise ValueError("resample runs on the GPU only (HIP kernel, no CPU path): move the audio to the device first")
    if waveform.dtype != torch.float32:
        raise TypeError(f"resample takes float32 audio, got {waveform.dtype}")
    if waveform.dim() == 0:
        raise ValueError("resample needs (..., time) audio")
    tab, table, first = _device_table(o, n, lowpass_filter_width, rolloff, waveform.device)
    L = waveform.shape[-1]
    Lo = tab.output_length(L)
    y = torch.empty(waveform.shape[:-1] + (Lo,), dtype=torch.float32, device=waveform.device)
    if y.numel() == 0:
        return y
    x, xs = _rows(waveform)
    with torch.cuda.device(waveform.device):
        _lib.call("xsq_resample", x.data_ptr(), xs, x.shape[0], L, y.data_ptr(), Lo, Lo, table.data_ptr(), first.data_ptr(), o, n, tab.span,
                  tab.width, _lib.stream_ptr())
    return y


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample for the sinc / Hann method, on ROCm tensors."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method: str = "sinc_interp_hann",
                 lowpass_filter_width: int = 6, rolloff: float = 0.99, beta=None, *, dtype=None):
        super().__init__()
        if resampling_method not in METHODS:
            raise ValueError(f"resampling_method {resampling_method!r}: only {METHODS} (Hann window) are implemented")
        if dtype not in (None, torch.float32):
            raise ValueError(f"dtype {dtype}: the resampler runs in float32")
        self.orig_freq, self.new_freq = _rates(orig_freq, new_freq)
        self.resampling_method = resampling_method
        self.lowpass_filter_width = int(lowpass_filter_width)
        self.rolloff = float(rolloff)
        if self.lowpass_filter_width <= 0 or not (0 < self.rolloff <= 1):
            raise ValueError(f"lowpass_filter_width {lowpass_filter_width} / rolloff {rolloff}")

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        if self.orig_freq == self.new_freq:
            return waveform
        return resample(waveform, self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
