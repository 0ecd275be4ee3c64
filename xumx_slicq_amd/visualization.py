"""The sliCQT spectrogram: overlap-add, dB, colour scale and raster on the device (csrc/spectrogram.hip).

Counterpart of the reference's ``visualization.py`` (``overlap_add_slicq`` :13-35, ``blockwise_spectrogram`` :38-116,
``visualization_main`` :119-229).  The reference overlap-adds in a Python loop, takes ``torch.quantile`` of a whole block and
hands every coefficient to matplotlib; here the coefficients stay where the forward transform left them and only the picture,
``nbands x width`` floats, leaves the device.  DESIGN.md section 4.14 has the full definition; in short, for block b of a plan
(coefficients (B, 2, F_b, S, T_b), hop h_b = T_b / 2, input of n samples):

  * overlap-add: ``ola[p] = sum_i x[i, p - i h_b]``; ``flatten=True``: the S slices side by side;
  * dB: ``20 log10 |.|``, h_b columns dropped at each end, THEN the mean over the two channels; |.| == 0 gives -inf;
  * truncation to ``N_b = min(int(T_b / L * n), (S - 1) h_b)`` columns (flatten: ``S T_b - T_b``).  The reference indexes the
    per-BAND list ``coef_factors()`` with the BLOCK index (visualization.py:204,220); here a block's factor is its own T_b / L;
  * colour scale: ``vmax`` = the 0.999 quantile (torch's "linear" interpolation) of the full-resolution dB values, -inf
    counting as a value, from an exact radix select on the device and a float64 lerp on the host; ``vmin = vmax - 120``;
  * raster (an extension: the reference draws one figure per block): one image (B, nbands, W), row = band; row f of block b,
    column w = max of the block's dB columns ``[w N_b // W, max(lo + 1, (w + 1) N_b // W))``.

ROCm tensors only: a CPU tensor raises ``XsqError``.  Every launch goes to the caller's current stream.

    python -m xumx_slicq_amd.visualization --input-wav track.wav --out-dir plots [--width 2560] [--per-block] [--flatten]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .plan import SliCQPlan, scale_frequencies

CMAPS = ("hot", "gray")


# ---- host-only arithmetic -------------------------------------------------------------------------------------------------
def block_columns(plan: SliCQPlan, n: int, S: int, flatten: bool = False) -> List[int]:
    """N_b per block: ``min(int((T_b / L) * n), (S - 1) h_b)``, flatten ``min(..., S T_b - T_b)`` -- the first factor in
    Python float arithmetic exactly as the reference writes it (visualization.py:57,79), with the block's own T_b / L."""
    n, S = int(n), int(S)
    out = []
    for (_, _F, T) in plan.blocks:
        ncoefs = int((T / plan.L) * n)
        most = S * T - T if flatten else (S - 1) * (T // 2)
        out.append(min(ncoefs, most))
    return out


def raster_ranges(N: int, W: int) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) int64 arrays of W entries: pixel w pools the columns [lo[w], hi[w]) of a row of N."""
    N, W = int(N), int(W)
    if N < 1 or W < 1:
        raise ValueError(f"raster_ranges: N={N}, W={W}: both at least 1")
    w = np.arange(W, dtype=np.int64)
    lo = (w * N) // W
    hi = np.maximum(lo + 1, ((w + 1) * N) // W)
    return lo, hi


def quantile_ranks(N: int, q: float) -> Tuple[int, int, float]:
    """(k_lo, k_hi, t): the q-quantile of N values with "linear" interpolation lies a fraction t of the way from the k_lo-th
    to the k_hi-th smallest (0-based): floor and ceil of q (N - 1)."""
    N, q = int(N), float(q)
    if N < 1 or not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile_ranks: N={N}, q={q}: N at least 1 and 0 <= q <= 1")
    pos = q * (N - 1)
    lo = min(int(math.floor(pos)), N - 1)
    hi = min(int(math.ceil(pos)), N - 1)
    return lo, hi, pos - lo


def quantile_lerp(v_lo: float, v_hi: float, t: float) -> float:
    """float64 lerp between two order statistics, the two-sided form numpy and torch use.  Equal ends are returned as they
    are and a lower end of -inf gives -inf: the form alone would make inf - inf = NaN of both."""
    a, b, t = float(v_lo), float(v_hi), float(t)
    if a == b or t == 0.0 or a == -math.inf:
        return a
    d = b - a
    return a + d * t if t < 0.5 else b - d * (1.0 - t)


def band_frequencies(plan: SliCQPlan) -> np.ndarray:
    """(nbands,) float64, Hz: 0 for the DC band, the scale's centre frequencies kept by the plan (0 < f < fs / 2), fs / 2."""
    f, _q = scale_frequencies(plan.scale, plan.fmin, plan.fmax, plan.fbins, plan.fgamma)
    f = f.double().numpy()
    nyq = plan.fs / 2.0
    f = f[(f > 0) & (f < nyq)]
    out = np.concatenate(([0.0], f, [nyq]))
    assert len(out) == plan.nbands, (len(out), plan.nbands)
    return out


def colormap(name: str, x: np.ndarray) -> np.ndarray:
    """x in [0, 1] -> (..., 3) uint8.  ``hot``: the piecewise-linear ramp black - red - yellow - white (red rises over the
    first 3/8, green over the next 3/8, blue over the last 1/4); ``gray``: the value itself."""
    x = np.asarray(x, dtype=np.float64)
    if name == "hot":
        rgb = np.stack([x / 0.375, (x - 0.375) / 0.375, (x - 0.75) / 0.25], axis=-1)
    elif name == "gray":
        rgb = np.stack([x, x, x], axis=-1)
    else:
        raise ValueError(f"cmap {name!r}: one of {CMAPS}")
    return np.rint(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)


def save_png(path: str, image, vmin: float, vmax: float, cmap: str = "hot") -> None:
    """``image`` (rows = bands, W) in dB -> 8-bit RGB PNG, low frequencies at the bottom.  Non-finite pixels and pixels below
    ``vmin`` take the lowest colour, finite pixels above ``vmax`` the highest.  zlib and struct only."""
    a = image.detach().cpu().numpy() if isinstance(image, Tensor) else np.asarray(image)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"save_png: expected one (rows, width) image, got {a.shape}")
    a = a.astype(np.float64)
    span = float(vmax) - float(vmin)
    x = np.zeros(a.shape, dtype=np.float64)
    if math.isfinite(span) and span > 0.0 and math.isfinite(float(vmin)):
        ok = np.isfinite(a)
        with np.errstate(invalid="ignore", over="ignore"):
            x = np.where(ok, np.clip((a - float(vmin)) / span, 0.0, 1.0), 0.0)
    rgb = colormap(cmap, x)[::-1]                                  # band 0 is the LAST row of the file
    rows, width = a.shape
    raw = np.concatenate([np.zeros((rows, 1), dtype=np.uint8), rgb.reshape(rows, width * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, rows, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ---- device side ----------------------------------------------------------------------------------------------------------
def _i32(values: Sequence[int]) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(list(values), dtype=np.int32))


def _need_device(t: Tensor, what: str) -> None:
    if not isinstance(t, Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, Tensor) else type(t).__name__
        raise _lib.XsqError(f"{what} runs on a ROCm device only (got '{where}'); there is no CPU fallback")


def _aligned(arena: Tensor) -> Tensor:
    return arena if arena.data_ptr() % 16 == 0 else arena.clone()


def overlap_add_slicq(slicq: Tensor, flatten: bool = False) -> Tensor:
    """The reference's signature: ``slicq`` (C, F, S, T) complex, or its real view (..., F, S, T, 2); returns the same kind,
    (C, F, (S + 1) T / 2) -- ``flatten``: (C, F, S T).  Bit for bit the reference's loop."""
    _need_device(slicq, "overlap_add_slicq")
    as_complex = slicq.is_complex()
    x = torch.view_as_real(slicq) if as_complex else slicq
    if x.dim() < 4 or x.shape[-1] != 2 or x.dtype != torch.float32:
        raise ValueError(f"overlap_add_slicq: expected (C, F, S, T) complex64 or (..., F, S, T, 2) float32; got {tuple(slicq.shape)} {slicq.dtype}")
    lead, (F, S, T) = tuple(x.shape[:-4]), (int(v) for v in x.shape[-4:-1])
    if T % 4:
        raise ValueError(f"overlap_add_slicq: T = {T}; every plan has T % 4 == 0 and the kernel loads half-slices 16 bytes at a time")
    BC = int(np.prod(lead)) if lead else 1
    x = _aligned(x.contiguous())
    Fa, Ta = _i32([F]), _i32([T])
    with torch.cuda.device(x.device):
        size = int(_lib.lib.xsq_spectrogram_overlap_add_size(1, Fa.ctypes.data, Ta.ctypes.data, BC, S, int(flatten)))
        out = torch.empty(size, dtype=torch.float32, device=x.device)
        _lib.call("xsq_spectrogram_overlap_add", 1, Fa.ctypes.data, Ta.ctypes.data, x.data_ptr(), BC, S, int(flatten), out.data_ptr(),
                  _lib.stream_ptr())
    out = out.view(*lead, F, -1, 2)
    return torch.view_as_complex(out) if as_complex else out


def overlap_add_blocks(X_list: Sequence[Tensor], base, flatten: bool = False) -> List[Tensor]:
    """``overlap_add_slicq`` of every block of what ``NSGT_SL`` returned, in one launch over the arena: per block
    (*lead, F_b, (S + 1) T_b / 2, 2) fp32 (flatten: (*lead, F_b, S T_b, 2)), views of one allocation."""
    X_list = list(X_list)
    for X in X_list:
        _need_device(X, "overlap_add_blocks")
    table = base.nsgt.table
    arena, lead, S = table.as_arena(X_list)
    arena = _aligned(arena)
    BC = int(np.prod(lead)) if lead else 1
    Fa, Ta = _i32(F for F, _ in table.shapes), _i32(T for _, T in table.shapes)
    with torch.cuda.device(arena.device):
        size = int(_lib.lib.xsq_spectrogram_overlap_add_size(len(Fa), Fa.ctypes.data, Ta.ctypes.data, BC, S, int(flatten)))
        out = torch.empty(size, dtype=torch.float32, device=arena.device)
        _lib.call("xsq_spectrogram_overlap_add", len(Fa), Fa.ctypes.data, Ta.ctypes.data, arena.data_ptr(), BC, S, int(flatten),
                  out.data_ptr(), _lib.stream_ptr())
    views, off = [], 0
    for F, T in table.shapes:
        Lout = S * T if flatten else (S + 1) * (T // 2)
        views.append(out[off: off + 2 * BC * F * Lout].view(*lead, F, Lout, 2))
        off += 2 * BC * F * Lout
    return views


class _Geometry:
    """Block table of one call as the entry points take it, and the views of the flat dB buffer."""

    def __init__(self, plan: SliCQPlan, n: int, S: int, B: int, flatten: bool):
        self.plan, self.n, self.S, self.B, self.flatten = plan, int(n), int(S), int(B), bool(flatten)
        self.columns = block_columns(plan, n, S, flatten)
        if min(self.columns) < 1:
            k = int(np.argmin(self.columns))
            raise ValueError(f"{n} samples give block {k} (T = {plan.blocks[k][2]}, slice length {plan.L}) no column: the signal is too short for a picture")
        self.F, self.T, self.N = _i32(F for (_, F, _) in plan.blocks), _i32(T for (_, _, T) in plan.blocks), _i32(self.columns)
        self.per_item = int(sum(int(F) * int(N) for F, N in zip(self.F, self.N)))

    def views(self, db: Tensor) -> List[Tensor]:
        out, off = [], 0
        for F, N in zip(self.F.tolist(), self.N.tolist()):
            out.append(db[off: off + self.B * F * N].view(self.B, F, N))
            off += self.B * F * N
        return out


def _db(geo: _Geometry, arena: Tensor) -> Tensor:
    arena = _aligned(arena)
    with torch.cuda.device(arena.device):
        db = torch.empty(geo.B * geo.per_item, dtype=torch.float32, device=arena.device)
        _lib.call("xsq_spectrogram_db", len(geo.F), geo.F.ctypes.data, geo.T.ctypes.data, geo.N.ctypes.data, arena.data_ptr(), geo.B, geo.S,
                  int(geo.flatten), db.data_ptr(), _lib.stream_ptr())
    return db


def order_statistics(values: Tensor, q: float) -> Tuple[np.ndarray, float]:
    """values (B, N) fp32 on the device -> ((B, 2) float32 on the host: the two order statistics around the q-quantile of
    every row, exact; the lerp weight).  ``quantile`` finishes the job."""
    _need_device(values, "order_statistics")
    if values.dim() != 2 or values.dtype != torch.float32 or values.shape[1] < 1:
        raise ValueError(f"order_statistics: expected (B, N >= 1) float32; got {tuple(values.shape)} {values.dtype}")
    B, N = int(values.shape[0]), int(values.shape[1])
    return _order_stats(_i32([1]), _i32([N]), values.contiguous(), B, q)


def _order_stats(F: np.ndarray, N: np.ndarray, db: Tensor, B: int, q: float) -> Tuple[np.ndarray, float]:
    total = int(sum(int(f) * int(n) for f, n in zip(F, N)))
    k_lo, k_hi, t = quantile_ranks(total, q)
    with torch.cuda.device(db.device):
        ws = torch.empty(int(_lib.lib.xsq_spectrogram_order_workspace(B)), dtype=torch.uint8, device=db.device)
        out = torch.empty(B, 2, dtype=torch.float32, device=db.device)
        _lib.call("xsq_spectrogram_order_stats", len(F), F.ctypes.data, N.ctypes.data, db.data_ptr(), B, k_lo, k_hi, out.data_ptr(),
                  ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        return out.cpu().numpy(), t


def quantile(values: Tensor, q: float) -> np.ndarray:
    """(B,) float64: the q-quantile of every row of ``values`` (B, N), "linear" interpolation, any N (no 2^24 limit)."""
    stats, t = order_statistics(values, q)
    return np.asarray([quantile_lerp(lo, hi, t) for lo, hi in stats.astype(np.float64)], dtype=np.float64)


def _raster(geo: _Geometry, db: Tensor, width: int) -> Tensor:
    with torch.cuda.device(db.device):
        image = torch.empty(geo.B, geo.plan.nbands, int(width), dtype=torch.float32, device=db.device)
        _lib.call("xsq_spectrogram_raster", len(geo.F), geo.F.ctypes.data, geo.N.ctypes.data, db.data_ptr(), geo.B, int(width),
                  image.data_ptr(), _lib.stream_ptr())
    return image


def _geometry_of(X_list: Sequence[Tensor], n: int, base, flatten: bool):
    eng = base.nsgt
    X_list = list(X_list)
    for X in X_list:
        _need_device(X, "blockwise_db")
    arena, lead, S = eng.table.as_arena(X_list)
    if len(lead) != 2 or lead[1] != 2:
        raise ValueError(f"blockwise_db: expected blocks (B, 2, F, S, T, 2); got a leading shape {lead}")
    return _Geometry(eng.plan, n, S, lead[0], flatten), arena


def blockwise_db(X_list: Sequence[Tensor], n: int, base, flatten: bool = False) -> List[Tensor]:
    """What ``NSGT_SL`` returned for an input of ``n`` samples -> per block (B, F_b, N_b) fp32 dB, spanning the whole signal in
    time: one pass over the arena (zero-copy through ``BlockTable.as_arena``).  ``base``: the ``NSGTBase`` of the transform."""
    geo, arena = _geometry_of(X_list, n, base, flatten)
    return geo.views(_db(geo, arena))


@dataclass
class Spectrogram:
    image: Tensor                          # (B, nbands, width) fp32 dB on the device, row = band
    vmax: np.ndarray                       # (B,) float64
    vmin: np.ndarray                       # (B,) float64: vmax - dynamic_range
    freqs: np.ndarray                      # (nbands,) Hz, 0 for the DC band
    duration: float                        # seconds
    columns: List[int]                     # N_b
    blocks: Optional[List[Tensor]] = None  # per_block: (B, F_b, N_b) dB at full resolution
    block_vmax: Optional[np.ndarray] = None  # per_block: (nblocks, B) float64


def spectrogram(audio: Tensor, base, width: int = 2560, flatten: bool = False, q: float = 0.999, dynamic_range: float = 120.0,
                per_block: bool = False) -> Spectrogram:
    """audio (B, 2, n) on the device -> the picture of its sliCQT under ``base`` (an ``NSGTBase``): forward transform, one dB
    pass, the colour scale from the full-resolution dB values of each batch item, the raster."""
    _need_device(audio, "spectrogram")
    if audio.dim() != 3 or audio.shape[1] != 2 or audio.shape[2] < 1:
        raise ValueError(f"spectrogram: expected audio (B, 2, n); got {tuple(audio.shape)}")
    if int(width) < 1:
        raise ValueError(f"spectrogram: width {width}: at least one column")
    eng = base.nsgt
    B, n = int(audio.shape[0]), int(audio.shape[2])
    geo = _Geometry(eng.plan, n, eng.plan.num_slices(n), B, flatten)          # refuses a signal too short before anything runs
    with torch.no_grad():
        arena, _lead, S = eng.forward(audio)
        assert S == geo.S
        db = _db(geo, arena)
        image = _raster(geo, db, width)
        stats, t = _order_stats(geo.F, geo.N, db, B, q)
        vmax = np.asarray([quantile_lerp(lo, hi, t) for lo, hi in stats.astype(np.float64)], dtype=np.float64)
        out = Spectrogram(image=image, vmax=vmax, vmin=vmax - float(dynamic_range), freqs=band_frequencies(eng.plan),
                          duration=n / float(eng.plan.fs), columns=list(geo.columns))
        if per_block:
            out.blocks = geo.views(db)
            rows = []
            for blk in out.blocks:
                s, tb = _order_stats(_i32([blk.shape[1]]), _i32([blk.shape[2]]), blk, B, q)
                rows.append([quantile_lerp(lo, hi, tb) for lo, hi in s.astype(np.float64)])
            out.block_vmax = np.asarray(rows, dtype=np.float64)
    return out


# ---- command line -----------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m xumx_slicq_amd.visualization", description="sliCQT spectrogram of a wav file, computed on the GPU")
    p.add_argument("--input-wav", type=str, required=True, help="input file")
    p.add_argument("--sr", type=int, default=44100, help="sample rate of the sliCQT; a file at another rate is resampled on the GPU (default=%(default)s)")
    p.add_argument("--cmap", type=str, default="hot", choices=CMAPS, help="colour map")
    p.add_argument("--fscale", choices=("mel", "bark", "Bark"), default="Bark", help="frequency scale")
    p.add_argument("--fbins", type=int, default=262, help="number of frequency bins (default=%(default)s)")
    p.add_argument("--fmin", type=float, default=32.9, help="minimum frequency in Hz (default=%(default)s)")
    p.add_argument("--flatten", action="store_true", help="slices side by side instead of overlap-added")
    p.add_argument("--out-dir", type=str, default=".", help="where <name>.png and <name>.json go")
    p.add_argument("--width", type=int, default=2560, help="columns of the picture (default=%(default)s)")
    p.add_argument("--per-block", action="store_true", help="also one picture per block, <name>-block-<i>.png, on the block's own colour scale")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    p = build_parser()
    a = p.parse_args(argv)
    if a.sr <= 0:
        p.error(f"--sr {a.sr}: a positive sample rate")
    if a.fbins < 2:
        p.error(f"--fbins {a.fbins}: at least two bins")
    if a.width < 1:
        p.error(f"--width {a.width}: at least one column")
    if not a.fmin > 0.0:
        p.error(f"--fmin {a.fmin}: above 0 Hz")
    if a.fmin >= a.sr / 2.0:
        p.error(f"--fmin {a.fmin} Hz is not below the Nyquist frequency of --sr {a.sr} ({a.sr / 2.0} Hz)")
    if not os.path.exists(a.input_wav):
        p.error(f"input file '{a.input_wav}' not found")
    if os.path.exists(a.out_dir) and not os.path.isdir(a.out_dir):
        p.error(f"--out-dir '{a.out_dir}' exists and is no directory")
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import audio as xaudio
    from .scoring import to_jsonable
    from .transforms import NSGTBase
    try:
        base = NSGTBase(a.fscale.lower(), a.fbins, a.fmin, fmax=a.sr / 2.0, fs=float(a.sr))
    except (ValueError, AssertionError) as e:
        raise SystemExit(f"no sliCQT plan for --fscale {a.fscale} --fbins {a.fbins} --fmin {a.fmin} --sr {a.sr}: {e}")
    if not torch.cuda.is_available():
        raise _lib.XsqError("the spectrogram is computed on a ROCm device only; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    sig, rate = xaudio.load_audio(a.input_wav)
    x = xaudio.preprocess_audio(sig.to(dev), rate, float(a.sr))
    sp = spectrogram(x, base, width=a.width, flatten=a.flatten, per_block=a.per_block)
    os.makedirs(a.out_dir, exist_ok=True)
    name = os.path.splitext(os.path.basename(a.input_wav))[0]
    image = sp.image[0].cpu().numpy()
    save_png(os.path.join(a.out_dir, name + ".png"), image, sp.vmin[0], sp.vmax[0], a.cmap)
    info = {"vmax": float(sp.vmax[0]), "vmin": float(sp.vmin[0]), "freqs": sp.freqs, "duration": sp.duration, "width": a.width,
            "nbands": int(image.shape[0]), "flatten": bool(a.flatten), "columns": sp.columns}
    if a.per_block:
        row = 0
        for i, (_, F, _T) in enumerate(base.plan.blocks):
            vm = float(sp.block_vmax[i, 0])
            save_png(os.path.join(a.out_dir, f"{name}-block-{i}.png"), image[row: row + F], vm - 120.0, vm, a.cmap)
            row += F
        info["block_vmax"] = sp.block_vmax[:, 0]
    with open(os.path.join(a.out_dir, name + ".json"), "w") as f:
        json.dump(to_jsonable(info), f)
    print(f"{name}: {image.shape[0]} bands x {a.width} columns, {sp.duration:.2f} s, vmax {sp.vmax[0]:.2f} dB -> {os.path.join(a.out_dir, name + '.png')}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
