"""Device-resident training data: the counterpart of ``MUSDBDataset`` (xumx_slicq_v2/data.py:211-393) and
of the ``DataLoader`` around it (training.py:329-338) for stems that stay in HBM.

The reference decodes every excerpt from disk in worker processes, augments it on the CPU and ships B x (1 + 4) x 2 rows
per step to the device.  Here the stems of all tracks are uploaded once (``DeviceDataset``: fp32, or the files' 16-bit
PCM), each epoch's excerpts are drawn on the host as one small table (``draw_epoch``), and each batch is built by ONE
launch of ``xsq_batch_assemble`` (csrc/batch.hip) from the table's rows of that step: slice, gain, channel swap, stack and
stem sum, with the arithmetic of ``audio * g`` (data.py:188) followed by ``stems.sum(0)`` (data.py:364).

Departures from the reference, all deliberate:
  * only its TRAINING configuration is drawn: ``random_track_mix=True``, the ``gain`` and ``channelswap`` augmentations,
    ``fixed_start=-1`` (data.py:219-235);
  * excerpt starts are drawn in samples, uniform over the integers [0, max(len - n, 0)], not in seconds;
  * a track shorter than the excerpt is zero-padded at its tail (the reference's ``torch.stack`` fails on it);
  * the generator is ``numpy.random.default_rng([seed, epoch])``: the same (seed, epoch) gives the same table on any
    machine.  The reference's ``random`` / ``torch.rand`` streams run inside DataLoader workers and are not reproducible;
  * the mix of a validation track is the fp32 sum of its stems (``mixture.wav`` is not read: MUSDB18-HQ mixtures are the
    stem sums up to 16-bit rounding), and validation tracks are handed out in pieces (``pieces``).

There is no CPU path for ``batch`` / ``pieces``: a pool on the CPU (``device="cpu"``) can be built and inspected, nothing more.
"""
from __future__ import annotations

import os
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

SAMPLE_RATE = 44100
NBUFFERS = 5            # Trainer.step(wait=False) keeps the inputs of its last four steps alive


def _round8(n: int) -> int:
    return (int(n) + 7) // 8 * 8


class DrawTable:
    """One epoch's excerpts: ``records`` int32 (items, 4 source columns, 4) = track, start, gain (fp32 bits), swap, and
    the same on the device (``dev``), where step k's batch is the ``batch_size`` items from k * batch_size on (the last
    batch is ragged, as the reference's DataLoader leaves it)."""

    def __init__(self, records: np.ndarray, batch_size: int, n: int, dev: Optional[Tensor]):
        self.records, self.batch_size, self.n, self.dev = records, int(batch_size), int(n), dev

    @property
    def nitems(self) -> int:
        return int(self.records.shape[0])

    @property
    def nsteps(self) -> int:
        return -(-self.nitems // self.batch_size)

    def __len__(self) -> int:
        return self.nsteps

    def items_of(self, step: int) -> int:
        if not 0 <= step < self.nsteps:
            raise IndexError(f"step {step} of an epoch of {self.nsteps} batches")
        return min(self.batch_size, self.nitems - step * self.batch_size)

    @property
    def gains(self) -> np.ndarray:
        return self.records[..., 2].view(np.float32)


def validate_table(records: np.ndarray, lengths: Sequence[int], n: int) -> None:
    """What ``xsq_batch_assemble`` trusts: 0 <= track < ntracks, 0 <= start, and start + n <= len unless the track is
    shorter than n, which must start at 0; swap is 0 or 1 and the gain is finite.  ValueError otherwise."""
    r = np.asarray(records)
    if r.dtype != np.int32 or r.ndim != 3 or r.shape[1:] != (4, 4):
        raise ValueError(f"a draw table is int32 (items, 4, 4); got {r.dtype} {r.shape}")
    lens = np.asarray(lengths, dtype=np.int64)
    track, start = r[..., 0].astype(np.int64), r[..., 1].astype(np.int64)
    if n < 1 or n >= 2 ** 31:
        raise ValueError(f"excerpt length {n} (1 .. 2^31 - 1)")
    if track.size and (track.min() < 0 or track.max() >= len(lens)):
        raise ValueError(f"draw table: track index outside [0, {len(lens)})")
    ln = lens[track]
    ok = (start >= 0) & np.where(ln >= n, start + n <= ln, start == 0)
    if not ok.all():
        i = np.argwhere(~ok)[0]
        raise ValueError(f"draw table: item {i[0]} column {i[1]} reads [{start[tuple(i)]}, +{n}) of a track of {ln[tuple(i)]} samples")
    if ((r[..., 3] != 0) & (r[..., 3] != 1)).any():
        raise ValueError("draw table: swap must be 0 or 1")
    if not np.isfinite(r[..., 2].view(np.float32)).all():
        raise ValueError("draw table: gains must be finite")


class DeviceDataset:
    """The stems of a set of tracks in one device allocation.

    Pool layout: track t is 8 rows of ``lengths[t]`` samples, row (source column s, channel c) at element
    ``offsets[t] + (2 s + c) * round_up(len, 8)``; offsets are multiples of 8, so every row starts 16-byte aligned in
    both storages, and the padding behind a row is zero.  ``storage="pcm16"`` keeps the files' int16 (value / 32768 on
    read, exact), ``"fp32"`` floats.

    ``sources`` is the column order and with it the summation order of the mix.  It is meant to be musdb's
    ``setup["sources"]`` order (data.py:324), which could not be checked against the musdb package when this was
    written: it is an attribute so that it can be corrected in one place.  ``target_of_column`` maps the columns to the
    target planes of y, ``Separator.sources`` = bass, vocals, other, drums (data.py:381-389)."""

    sources: Tuple[str, ...] = ("vocals", "drums", "bass", "other")
    targets: Tuple[str, ...] = ("bass", "vocals", "other", "drums")
    sample_rate = float(SAMPLE_RATE)

    def __init__(self, lengths: Sequence[int], loader, storage: str = "pcm16", device="cuda", names=None):
        """``loader(t)`` -> (8, lengths[t]) array of the storage's dtype, rows (source column, channel).  Use the
        ``from_arrays`` / ``from_directory`` constructors."""
        if storage not in ("pcm16", "fp32"):
            raise ValueError(f"storage {storage!r}: 'pcm16' or 'fp32'")
        if len(lengths) == 0:
            raise ValueError("a dataset needs at least one track")
        self.storage, self.device = storage, torch.device(device)
        self.lengths = np.asarray([int(n) for n in lengths], dtype=np.int64)
        if (self.lengths < 1).any() or (self.lengths >= 2 ** 31).any():
            raise ValueError("track lengths must lie in [1, 2^31)")
        strides = np.asarray([_round8(n) for n in self.lengths], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(8 * strides)[:-1]]).astype(np.int64)
        self.names = list(names) if names is not None else [f"track{t}" for t in range(len(self.lengths))]
        dtype = torch.int16 if storage == "pcm16" else torch.float32
        self.pool = torch.zeros(int(8 * strides.sum()), dtype=dtype, device=self.device)
        for t, (off, n, st) in enumerate(zip(self.offsets, self.lengths, strides)):
            rows = np.ascontiguousarray(loader(t))
            if rows.shape != (8, n) or rows.dtype != (np.int16 if storage == "pcm16" else np.float32):
                raise ValueError(f"track {t}: expected (8, {n}) {storage} rows, got {rows.shape} {rows.dtype}")
            self.pool[off:off + 8 * st].view(8, st)[:, :n].copy_(torch.from_numpy(rows))
        self.tracks = torch.from_numpy(np.stack([self.offsets, self.lengths], axis=1).copy()).to(self.device)
        self.target_of_column = tuple(self.targets.index(s) for s in self.sources)
        self._toc = torch.tensor(self.target_of_column, dtype=torch.int32, device=self.device)
        self._bufs: Dict[Tuple[int, int], list] = {}

    def __len__(self) -> int:
        return len(self.lengths)

    # -- constructors ------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, tracks: Sequence[Dict[str, np.ndarray]], storage: str = "pcm16", device="cuda", names=None):
        """``tracks``: a list of {source name: (2, len) array}.  int16 arrays go to pcm16 storage as they are (and to
        fp32 storage as value / 32768); float arrays under ``storage="pcm16"`` raise ValueError -- nothing is quantised
        silently."""
        stems, lengths = [], []
        for t, tr in enumerate(tracks):
            missing = [s for s in cls.sources if s not in tr]
            if missing:
                raise ValueError(f"track {t}: no {missing} (sources are {cls.sources})")
            rows = [np.asarray(tr[s].detach().cpu().numpy() if isinstance(tr[s], Tensor) else tr[s]) for s in cls.sources]
            if any(r.ndim != 2 or r.shape != (2, rows[0].shape[1]) for r in rows):
                raise ValueError(f"track {t}: every source is a (2, len) array of one length; got {[r.shape for r in rows]}")
            stems.append(np.concatenate([_to_storage(r, storage, f"track {t}") for r in rows], axis=0))
            lengths.append(rows[0].shape[1])
        return cls(lengths, lambda t: stems[t], storage=storage, device=device, names=names)

    @classmethod
    def from_directory(cls, root: str, names: Optional[Sequence[str]] = None, storage: str = "pcm16", device="cuda"):
        """``<root>/<track>/{vocals,drums,bass,other}.wav`` (the MUSDB18-HQ layout) through ``audio.load_audio``.
        ``names``: the track directories to take, in this order (default: all of them, sorted).  Mono is duplicated and
        more than two channels are cut to two (data.py:199-208); a rate other than 44100 raises ValueError, as do stems
        of unequal length and, under ``storage="pcm16"``, files whose samples are not 16-bit values."""
        from .audio import load_audio, load_info
        if names is None:
            names = sorted(d for d in os.listdir(root)
                           if all(os.path.isfile(os.path.join(root, d, s + ".wav")) for s in cls.sources))
        names = list(names)
        lengths = []
        for name in names:
            infos = [load_info(os.path.join(root, name, s + ".wav")) for s in cls.sources]
            if any(i["samplerate"] != SAMPLE_RATE for i in infos):
                raise ValueError(f"{name}: sample rate {[i['samplerate'] for i in infos]}; the dataset is {SAMPLE_RATE} Hz")
            if len({i["samples"] for i in infos}) != 1:
                raise ValueError(f"{name}: stems of unequal length {[i['samples'] for i in infos]}")
            lengths.append(infos[0]["samples"])

        def load(t):
            rows = []
            for s in cls.sources:
                a = load_audio(os.path.join(root, names[t], s + ".wav"))[0].numpy()
                a = a[:2] if a.shape[0] > 2 else a
                a = np.repeat(a, 2, axis=0) if a.shape[0] == 1 else a
                rows.append(_to_storage(a, storage, f"{names[t]}/{s}.wav", from_file=True))
            return np.concatenate(rows, axis=0)

        return cls(lengths, load, storage=storage, device=device, names=names)

    # -- the epoch's table ---------------------------------------------------------------------
    def draw_epoch(self, seed: int, epoch: int, batch_size: int, seq_dur: float, samples_per_track: int = 64,
                   augment: bool = True) -> DrawTable:
        """The records of one epoch, validated and uploaded once: ``len(self) * samples_per_track`` items (data.py:392-393)
        of ``n = int(seq_dur * 44100)`` samples.  From ``numpy.random.default_rng([seed, epoch])``, four arrays of shape
        (items, 4 source columns) are drawn in this order:
          1. the track, ``integers(0, ntracks)`` (data.py:327);
          2. the start, ``integers(0, max(len - n, 0) + 1)`` of that track (data.py:340, in samples);
          3. the gain ``0.25 + k * 2^-23`` with ``k = integers(0, 2^23)``: fp32-exact, in [0.25, 1.25) (data.py:183-188);
          4. the swap bit, ``integers(0, 2)`` (data.py:191-196).
        ``augment=False`` stops after 2: gain 1, no swap."""
        n = int(seq_dur * SAMPLE_RATE)
        if batch_size < 1 or samples_per_track < 1 or n < 1:
            raise ValueError(f"batch_size {batch_size}, samples_per_track {samples_per_track}, {n} samples per excerpt")
        items = len(self) * int(samples_per_track)
        rng = np.random.default_rng([int(seed), int(epoch)])
        rec = np.zeros((items, 4, 4), dtype=np.int32)
        track = rng.integers(0, len(self), size=(items, 4))
        rec[..., 0] = track
        rec[..., 1] = rng.integers(0, np.maximum(self.lengths[track] - n, 0) + 1)
        gain = np.ones((items, 4), dtype=np.float32)
        if augment:
            gain = np.float32(0.25) + rng.integers(0, 1 << 23, size=(items, 4)).astype(np.float32) * np.float32(2.0 ** -23)
            rec[..., 3] = rng.integers(0, 2, size=(items, 4))
        rec[..., 2] = gain.astype(np.float32).view(np.int32)
        return self.table(rec, batch_size, n)

    def table(self, records: np.ndarray, batch_size: int, n: int) -> DrawTable:
        """Validates ``records`` (``validate_table``) and uploads them."""
        records = np.ascontiguousarray(records)
        validate_table(records, self.lengths, n)
        dev = torch.from_numpy(records).to(self.device) if self.device.type == "cuda" else None
        return DrawTable(records, batch_size, n, dev)

    # -- batches ---------------------------------------------------------------------------------
    def _buffers(self, B: int, n: int) -> Tuple[Tensor, Tensor]:
        ring = self._bufs.setdefault((B, n), [-1, []])
        if len(ring[1]) < NBUFFERS:
            ring[1].append((torch.empty(B, 2, n, dtype=torch.float32, device=self.device),
                            torch.empty(4, B, 2, n, dtype=torch.float32, device=self.device)))
            return ring[1][-1]
        ring[0] = (ring[0] + 1) % NBUFFERS
        return ring[1][ring[0]]

    def assemble(self, draws: Tensor, step: int, B: int, n: int, x: Tensor, y: Tensor) -> None:
        """One ``xsq_batch_assemble`` launch on the current stream: rows [step * B, (step + 1) * B) of the device table
        ``draws`` into x (B, 2, n) and y (4, B, 2, n), contiguous fp32 on the pool's device."""
        if self.device.type != "cuda":
            raise _lib.XsqError("batches are assembled on a ROCm device only; there is no CPU fallback")
        for t, shape in ((x, (B, 2, n)), (y, (4, B, 2, n))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.pool.device:
                raise ValueError(f"expected contiguous fp32 {shape} on {self.pool.device}; got {t.dtype} {tuple(t.shape)} on {t.device}")
        if draws.dtype != torch.int32 or draws.device != self.pool.device or not draws.is_contiguous() \
                or draws.numel() < (step + 1) * B * 16:
            raise ValueError("the draw table must be a contiguous int32 device tensor holding the step's rows")
        with torch.cuda.device(self.device):
            _lib.call("xsq_batch_assemble", self.pool.data_ptr(), 1 if self.storage == "pcm16" else 0, self.tracks.data_ptr(), len(self),
                      draws.data_ptr(), step, B, n, self._toc.data_ptr(), x.data_ptr(), y.data_ptr(), _lib.stream_ptr())

    def batch(self, table: DrawTable, step: int, out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
        """(x (B, 2, n) mix, y (4, B, 2, n) targets) of step ``step`` of ``table``, in buffers the dataset owns and
        cycles through: a batch stays intact while the next ``NBUFFERS - 1`` are built.  ``out`` = (x, y): the caller's
        buffers instead."""
        B = table.items_of(step)
        x, y = out if out is not None else self._buffers(B, table.n)
        if B == table.batch_size:
            self.assemble(table.dev, step, B, table.n, x, y)
        else:                                              # the ragged last batch: its rows start where the full ones end
            self.assemble(table.dev.view(-1)[step * table.batch_size * 16:], 0, B, table.n, x, y)
        return x, y

    def pieces(self, i: int, chunk: int) -> Iterator[Tuple[Tensor, Tensor]]:
        """Track ``i`` whole, as consecutive pieces of ``chunk`` samples (the last one shorter): (x (1, 2, n),
        y (4, 1, 2, n)) with gain 1, no swap and the mix the fp32 stem sum -- the same kernel on a one-row table."""
        if not 0 <= i < len(self) or chunk < 1:
            raise ValueError(f"track {i} of {len(self)}, chunk {chunk}")
        length = int(self.lengths[i])
        starts = list(range(0, length, int(chunk)))
        rec = np.zeros((len(starts), 4, 4), dtype=np.int32)
        rec[..., 0], rec[..., 1], rec[..., 2] = i, np.asarray(starts, dtype=np.int32)[:, None], np.float32(1).view(np.int32)
        for k, s in enumerate(starts):                      # every piece ends inside the track
            validate_table(rec[k:k + 1], self.lengths, min(chunk, length - s))
        dev = torch.from_numpy(rec).to(self.device)
        for k, s in enumerate(starts):
            n = min(int(chunk), length - s)
            x, y = self._buffers(1, n)
            self.assemble(dev, k, 1, n, x, y)
            yield x, y


def _to_storage(a: np.ndarray, storage: str, what: str, from_file: bool = False) -> np.ndarray:
    """(2, len) samples as the pool keeps them.  int16 -> pcm16 as is, -> fp32 as value / 32768; floats -> fp32 as is;
    floats -> pcm16 only for a decoded 16-bit file (``from_file``), whose samples are k / 32768 exactly -- checked."""
    if a.dtype == np.int16:
        return a if storage == "pcm16" else a.astype(np.float32) / np.float32(32768.0)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"{what}: samples are int16 or floating point, not {a.dtype}")
    if storage == "fp32":
        return a.astype(np.float32)
    if not from_file:
        raise ValueError(f"{what}: floating-point samples under storage='pcm16' would be quantised; pass int16 or use storage='fp32'")
    q = a.astype(np.float64) * 32768.0
    if not (np.array_equal(q, np.rint(q)) and q.min(initial=0) >= -32768 and q.max(initial=0) <= 32767):
        raise ValueError(f"{what}: not 16-bit PCM; use storage='fp32'")
    return q.astype(np.int16)
