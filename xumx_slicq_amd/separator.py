"""Drop-in mirror of /root/reference/xumx_slicq_v2/separator.py (Separator,
load_target_models) for the ROCm backend.

Same class/function names, arguments, attribute names, output layout
(targets first: (4, nb_samples, 2, N)) and exceptions as
the reference's torch path.  The ONNX runtimes and the GitHub download are
outside the accelerated path.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import weakref
from collections import namedtuple
from pathlib import Path
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .model import Unmix
from .transforms import ComplexNorm, NSGTBase, make_filterbanks
from .weights import seeded_state_dict

# the reference's list (separator.py:29) plus the backend this package provides
_SUPPORTED_RUNTIMES = ["torch-cpu", "torch-cuda", "onnx-cpu", "onnx-cuda", "hip-rocm"]
_ACCELERATED = "hip-rocm"

# THE list of A/B switches, each a plain instance attribute of its owner that is absent by default (tests set and delete
# it).  name: (owner: the Separator or its Unmix ("model"), environment variable read per call while the attribute is absent
# -- None: there is none --, default -- its type is the type of every value read --, whether a change drops the captured
# forwards (True) or is captured beside them (False)).  ``switch`` reads them; ``Separator._graph_key`` iterates them.
SWITCHES = {
    "native": ("separator", "XSQ_NATIVE_FORWARD", True, True),
    "fuse_whiten": ("separator", "XSQ_FUSE_WHITEN", True, True),
    "fuse_phasemix": ("separator", "XSQ_FUSE_PHASEMIX", True, True),
    "packed_fft": ("separator", "XSQ_PACKED_FFT", False, True),
    "batch_chunks": ("separator", None, True, False),
    "overlap_tail": ("separator", None, True, False),
    "max_stack": ("separator", None, 8, False),
    "pass_streams": ("separator", None, 1, False),
    "max_item_slices": ("separator", None, 0, True),
    "wiener_masked": ("model", "XSQ_WIENER_MASKED", True, True),
    "niter_method": ("model", None, "auto", True),
    "winograd": ("model", None, 23, True),
    "precision": ("model", None, "fp32", False),
}
_ABSENT = object()
# the key of a captured forward: captures of one device that differ in ``coexist`` live side by side in the cache, one that
# differs from the current call in ``invalidating`` is stale
GraphKey = namedtuple("GraphKey", "device coexist invalidating")
_Native = namedtuple("_Native", "dev model d main cs max_stack cap")      # ``Separator._native_call``
# The dependency window of a mask in mix-phase mode, in slices (XSQ_STREAM_* of the C header): the mask of slice s
# reads the coefficients of s - back .. s + ahead, back by the conv type -- the causal stack's first layer is left-padded.
STREAM_BACK = {True: 3, False: 2}          # causal -> back
STREAM_AHEAD = 2


def switch(owner, name: str):
    """Value of switch ``name`` on ``owner``: the instance attribute when there is one, else its environment variable (read per
    call; "0" is off, anything else on), else the default.  KeyError for a name that ``SWITCHES`` does not list."""
    _, env, default, _ = SWITCHES[name]
    value = vars(owner).get(name, _ABSENT)         # (a plain instance attribute: no walk through nn.Module.__getattr__)
    if value is not _ABSENT:
        return type(default)(value)
    env = os.environ.get(env) if env else None
    return default if env is None else env != "0"


def _fp32(audio: Tensor) -> Tensor:
    return audio if audio.dtype == torch.float32 and audio.is_contiguous() else audio.contiguous().float()


def _set_wiener_options(separator, niter, softmask, residual):
    """The post-filter options of ``Separator.load`` / ``seeded_separator``: None leaves the model's own."""
    for name, value in (("niter", niter), ("softmask", softmask), ("residual", residual)):
        if value is not None:
            setattr(separator, name, value)


class Separator(nn.Module):
    sources = ["bass", "vocals", "other", "drums"]      # separator.py:48
    accepts_item_lists = True                           # demix_into takes a list of per-item tensors (sharding.ShardedDemixer)

    @classmethod
    def load(cls, chunk_size: int = 2621440, model_path: Optional[str] = None,
             runtime_backend: Optional[str] = _ACCELERATED, warmup: int = 0, realtime: bool = False,
             device: Union[str, torch.device] = "cuda", niter: Optional[int] = None, softmask: Optional[bool] = None,
             residual: Optional[bool] = None, dc_twins: bool = False, long_bands: bool = False, fgamma: float = 15.0):
        """separator.py:50-93.  ``niter``, ``softmask``, ``residual`` (extensions): the options of the Wiener post-filter, see the
        properties of the same names.  ``dc_twins``: accept a checkpoint whose plan has bands across DC and decode it with the
        reference's mirrored synthesis (``plan.build_plan``); the default refuses such a plan.  ``long_bands``: accept a checkpoint
        trained on ``cqlog`` or ``vqlog`` (``fgamma``: the offset of the latter's centres, unless the JSON names one) and run its
        bands above 320 samples on the FFT band engine."""
        if runtime_backend not in _SUPPORTED_RUNTIMES:
            raise ValueError(f"requested runtime backend {runtime_backend} not in {_SUPPORTED_RUNTIMES}")
        xumx_model, encoder, sample_rate = load_target_models(
            model_path, runtime_backend=runtime_backend, realtime=realtime, device=device, dc_twins=dc_twins,
            long_bands=long_bands, fgamma=fgamma)
        separator = cls(xumx_model=xumx_model, encoder=encoder, sample_rate=sample_rate,
                        runtime_backend=runtime_backend, chunk_size=chunk_size, device=device).to(device)
        separator.freeze()
        _set_wiener_options(separator, niter, softmask, residual)
        for _ in range(warmup):
            waveform = torch.rand((1, 2, int(100 * sample_rate)), dtype=torch.float32, device=device)
            separator.forward(waveform)
        return separator

    def __init__(self, xumx_model: Unmix = None, encoder: Tuple = None, runtime_backend: str = _ACCELERATED,
                 sample_rate: float = 44100.0, chunk_size: Optional[int] = 2621440, device: str = "cuda",
                 quiet: bool = False):
        super().__init__()
        if runtime_backend != _ACCELERATED:
            raise ValueError(f"this package provides the '{_ACCELERATED}' backend only (got {runtime_backend}); "
                             "use the reference for torch-*/onnx-*")
        self.device = device
        self.nb_channels = 2
        self.register_buffer("sample_rate", torch.as_tensor(sample_rate))
        self.chunk_size = chunk_size if chunk_size is not None else sys.maxsize
        self.xumx_model = xumx_model
        self.runtime_backend = runtime_backend
        self.nsgt, self.insgt, self.cnorm = encoder
        self.quiet = quiet
        self.sources = Separator.sources
        self._nws = _lib.Scratch()     # the workspaces of the native calls (``_native_ws``)

    @property
    def dc_twins(self) -> bool:
        """The plan was built with ``dc_twins=True``: the inverse transforms add the mirrored synthesis of the bands across DC.
        ``stream``, ``demix_into`` (sharding) and ``Trainer`` refuse such a separator."""
        return bool(getattr(self.nsgt.nsgt.plan, "dc_twins", False))

    @property
    def long_bands(self) -> bool:
        """The plan was built with ``long_bands=True``: the bands above 320 samples run on the FFT band engine, which opens the
        scales ``cqlog`` and ``vqlog``.  ``stream``, ``demix_into`` (sharding) and ``Trainer`` refuse such a separator."""
        return bool(getattr(self.nsgt.nsgt.plan, "long_bands", False))

    def freeze(self):
        for p in self.parameters():
            p.grad = None
        self.xumx_model.freeze()
        self.eval()

    @property
    def niter(self) -> int:
        """EM iterations of the Wiener post-filter of an offline model: the ``niter`` of the Open-Unmix family,
        ``iterations`` of norbert.wiener (the reference pins 1, phase.py:53-58).  Lives on the model (``Unmix.niter``), read
        per call; 0 = the mix-phase estimate.  A realtime (mix-phase) model has no EM and ignores it."""
        return int(getattr(self.xumx_model, "niter", 1))

    @niter.setter
    def niter(self, value: int):
        value = int(value)
        if value < 0:
            raise ValueError(f"niter must be >= 0 (got {value})")
        self.xumx_model.niter = value

    @property
    def softmask(self) -> bool:
        """Start the Wiener post-filter of an offline model from the ratio mask x v_j / (eps + sum_j v_j) instead of the mixture
        phase on v_j: ``use_softmask`` of norbert.wiener, ``softmask`` of the Open-Unmix family (the reference pins False).  Lives on
        the model (``Unmix.softmask``), read per call; with ``niter`` = 0 that start is the result."""
        return bool(getattr(self.xumx_model, "softmask", False))

    @softmask.setter
    def softmask(self, value: bool):
        self.xumx_model.softmask = bool(value)

    @property
    def residual(self) -> bool:
        """Add a fifth source to the Wiener post-filter of an offline model, relu(|x| - sum_j v_j): what the four target models
        do not explain (norbert.contrib.residual_model, ``residual`` of the Open-Unmix family).  ``forward``, ``forward_graphed``
        and ``forward_overlapped`` then return (5, nb_samples, 2, N), the residual last.  Lives on the model (``Unmix.residual``)."""
        return bool(getattr(self.xumx_model, "residual", False))

    @residual.setter
    def residual(self, value: bool):
        self.xumx_model.residual = bool(value)

    def _nb_sources(self) -> int:
        return 5 if self.residual else 4

    def _handle_key(self):
        """What the workspace sizes of a native call depend on besides its shape: the packed-parameter version of the model handle
        and the option set stored on it."""
        return (self.xumx_model._version(), self.softmask, self.residual)

    def _graph_key(self, audio_big: Tensor):
        """Everything a captured forward depends on besides the input values: shape and device, the chunking
        switches, the packed-parameter version of the model (captured kernels hold raw pointers into the
        xsq_model handle), the arithmetic mode and the post-filter / fusion switches read per call."""
        m = self.xumx_model
        # two switches enter as what the call makes of them (the fusion on an all-mix-phase model, ``_packed_fft``), not as read
        derived = {"fuse_phasemix": self._fused(), "packed_fft": self._packed_fft()}
        items = [(drops, (name, derived[name] if name in derived else switch(m if owner == "model" else self, name)))
                 for name, (owner, _, _, drops) in SWITCHES.items()]
        coexist, dropping = (tuple(kv for d, kv in items if d is drops) for drops in (False, True))
        return GraphKey(audio_big.device.index, (tuple(audio_big.shape), self.chunk_size) + coexist,
                        (m._version(), tuple(bool(b.realtime) for b in m.sliced_umx), self.niter, self.softmask, self.residual) + dropping)

    def drop_graphs(self):
        """Forget every captured forward (they hold raw pointers into the model handle and the workspaces)."""
        self.__dict__.pop("_graphs", None)

    def forward_graphed(self, audio_big: Tensor) -> Tensor:
        """``forward`` replayed from a HIP graph captured per input shape (launch-bound shapes: the
        2.2 s tail chunk or streaming-sized inputs spend more time between launches than inside them).
        The result tensor is owned by the graph and overwritten by the next call of the same shape.
        Graphs captured against an older parameter version / post-filter setting are dropped before the
        model handle they point into is rebuilt (``Unmix._model`` frees it)."""
        key = self._graph_key(audio_big)
        cache = self.__dict__.setdefault("_graphs", {})
        for k in [k for k in cache if k.device == key.device and k.invalidating != key.invalidating]:
            del cache[k]                              # stale: would replay against freed device memory
        entry = cache.get(key)
        wiener = self._native_mode(audio_big)
        if wiener is not None:
            audio_big = _fp32(audio_big)
        if entry is None:
            # native path: the captured kernels read the input through a DEVICE pointer slot (xsq_separator_forward_indirect),
            # so a replay follows the caller's tensor -- no copy of the input into a static buffer (85 MB for a 240 s track).
            # Module-API schedule (an A/B switch off its default): the captured launches hold the input's address, so the
            # input is copied into a static tensor as before.
            slot = torch.zeros(1, dtype=torch.int64, device=audio_big.device) if wiener is not None else None
            static_in = None if slot is not None else audio_big.clone()
            if slot is not None:
                slot.fill_(audio_big.data_ptr())
            call = (lambda: self._forward_native(audio_big, wiener, slot=slot)) if slot is not None else (lambda: self.forward(static_in))
            side = torch.cuda.Stream(device=audio_big.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):          # warm-up on a side stream: fills the shape-keyed caches
                for _ in range(2):
                    call()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = call()
            # the captured kernels hold raw pointers into the grow-only workspaces: keep those tensors
            # alive with the graph even if a later, larger call replaces them in their owners
            entry = cache[key] = [graph, static_in, static_out, self._scratch_tensors(), slot, audio_big.data_ptr()]
        graph, static_in, static_out, _keep, slot, last_ptr = entry
        if slot is None:
            static_in.copy_(audio_big)
        elif audio_big.data_ptr() != last_ptr:
            slot.fill_(audio_big.data_ptr())       # 8 bytes, one small launch on the replay's stream, in front of the replay
            entry[5] = audio_big.data_ptr()
        graph.replay()
        return static_out

    def _scratch_tensors(self) -> list:
        """Every live workspace a forward of this separator can have written through: those of the two transforms' engines,
        of the model, of the post-filter (``phase``) and of the native calls."""
        from . import phase
        pools = (self.insgt.nsgt.nsgt.scratch, self.nsgt.nsgt.nsgt.scratch, self.xumx_model.scratch, phase.SCRATCH, self._nws)
        return [ws for pool in {id(p): p for p in pools}.values() for ws in pool.tensors()]       # (the transforms share an engine)

    def _packed_fft(self) -> bool:
        """Packed-fp32 butterflies in the slice FFTs: a DIAGNOSTIC build option (csrc/Makefile PACKED_FFT=1), not part of
        the product library -- measured, they change nothing (the transforms are bound by their HBM phases, DESIGN.md
        section 4) and next to v_mfma_f32_16x16x32_bf16 waves of another stream the packed transform returned wrong values
        (tools/probe/pk_mfma_hazard.hip).  ``packed_fft = True`` / XSQ_PACKED_FFT=1 asks the library for them; the product
        build refuses with ``XsqError``.  A diagnostic build honours it only while no model or trainer of this process
        contracts on split-bf16 MFMAs."""
        want = switch(self, "packed_fft")
        eng = self.nsgt.nsgt.nsgt
        if not want and not eng._packed_fft:
            return False
        from .model import split_bf16_active
        on = want and not split_bf16_active()
        eng.set_packed_fft(on)
        self.insgt.nsgt.nsgt.set_packed_fft(on)
        return on

    def _fused(self) -> bool:
        """Mix-phase models: the CDAE writes the masks only and the inverse transform forms mask * X while it
        loads (same products, same order: bitwise equal to decoding the materialised estimates)."""
        return bool(switch(self, "fuse_phasemix") and all(bool(b.realtime) for b in self.xumx_model.sliced_umx))

    def _demix_py(self, out: Tensor, audio: Tensor, length: int, offsets: Tensor, group: int = 0):
        """One pass of the Python chunk loop over (B, 2, n) audio, a short chunk zero-padded to sllen/2 + 1 (separator.py:162-170):
        forward transform, CDAE + post-filter, inverse transform; packed channel (target, b, c) is written to
        out.view(-1)[offsets[target, b, c] : +length].  By default the analysis kernels also write the CDAE's whitened
        magnitude straight into the model's workspace (xsq_slicqt_forward_xin; same values as the separate magnitude pass,
        which is then skipped); ``fuse_whiten = False`` / XSQ_FUSE_WHITEN=0 restores it."""
        short = int(self.nsgt.nsgt.sllen / 2) + 1 - audio.shape[-1]
        if short > 0:
            audio = torch.cat([audio, torch.zeros((*audio.shape[:-1], short), device=audio.device, dtype=audio.dtype)], dim=-1)
        eng = self.nsgt.nsgt.nsgt
        if not switch(self, "fuse_whiten") or audio.dim() != 3 or audio.shape[1] != 2 or audio.device.type != "cuda":
            Xc, xin_ready = self.nsgt(audio), False
        else:
            S = eng.plan.num_slices(audio.shape[-1])
            ws, mean, scale, split = self.xumx_model.whitening_target(audio.device, audio.shape[0], S)
            arena, lead, S = eng.forward(audio, whiten=(ws.data_ptr(), mean, scale, split))
            Xc, xin_ready = eng.table.views(arena, lead, S), True
        eng = self.insgt.nsgt.nsgt
        offs = offsets.reshape(-1).contiguous()
        if self._fused():
            masks, X, B, S = self.xumx_model.masks_arena(Xc, xin_ready=xin_ready)
            eng.backward_masked(masks, X, 8 * B, 2 * B, S, length, out, offs)
            return
        Ylist = self.xumx_model(Xc, wiener_batch_group=group, xin_ready=xin_ready)
        arena, lead, S = eng.table.as_arena(list(Ylist))
        eng.backward(arena, offs.numel(), S, length, out=out, row_offsets=offs)

    def _input_rows(self, items):
        """Input row table (device int64, element offsets from items[0]) of a list of equally shaped (nb_samples, 2, n) fp32
        tensors on one device, or None when the list has to be packed: xsq_demix_pass then reads every work item where it
        lies -- chunk views of different tracks -- instead of through a torch.cat copy (84 MB per stacked pass of four
        full chunks).  Cached by the tensors' addresses and strides."""
        t0 = items[0]
        if len(items) < 2 or self._native_mode(t0) is None:
            return None
        for t in items:
            if (t.dim() != 3 or t.shape != t0.shape or t.dtype != torch.float32 or t.device != t0.device or t.stride(-1) != 1
                    or (t.data_ptr() - t0.data_ptr()) % 4):
                return None
        # the table has 2 * nb rows per item: nb (and the device) belong to the key, not only the addresses and strides
        key = (t0.device.index, int(t0.shape[0])) + tuple((t.data_ptr(), t.stride(0), t.stride(1)) for t in items)
        cache = self.__dict__.setdefault("_xrows", {})
        hit = cache.get(key)
        if hit is None:
            base = t0.data_ptr()
            rows = [(t.data_ptr() - base) // 4 + b * t.stride(0) + c * t.stride(1)
                    for t in items for b in range(t.shape[0]) for c in range(2)]
            if len(cache) > 4096:
                # kernels in flight on either stream may still read an evicted table (the allocator orders reuse on the
                # allocating stream only): wait for the device before the tables go.  Once per 4096 new item lists.
                torch.cuda.synchronize(t0.device)
                cache.clear()
            hit = cache[key] = torch.tensor(rows, dtype=torch.int64, device=t0.device)
        return hit

    @torch.no_grad()
    def demix_into(self, audio, out: Tensor, row_offsets: Tensor, group: int = 1):
        """One pass over ``audio`` (k * group, 2, n): k independent work items of n <= chunk_size samples each
        (chunks of any tracks -- no state crosses the reference's chunk loop, separator.py:153-229), ``group``
        = nb_samples of an item; or a LIST of k tensors (group, 2, n), read in place.  Four stems per item: ``residual`` is
        refused (ValueError).  The stems of packed channel
        (target, item*group + b, c) land at out.view(-1)[row_offsets[target, item*group + b, c] : + n] -- the hard concat
        of separator.py:231 by placement.  The Wiener window maximum keeps its per-item scope (quirk A13) through
        ``group``.  Building block of ``sharding.ShardedDemixer``; ``forward`` is the single-track case."""
        if self.residual:
            raise ValueError("demix_into places four stems per work item (row_offsets (4, B, 2)); residual = True writes five: "
                             "use forward, or switch residual off for the multi-track batch")
        if self.dc_twins:
            raise _lib.XsqError("demix_into / sharding: a plan with bands across DC (dc_twins = True) is served by forward, forward_graphed, "
                                "forward_overlapped and remix only")
        if self.long_bands:
            raise _lib.XsqError("demix_into / sharding: a plan with bands on the FFT band engine (long_bands = True) is served by forward, "
                                "forward_graphed, forward_overlapped and remix only")
        x_rows, keep = None, None
        if isinstance(audio, (list, tuple)):
            keep = list(audio)
            x_rows = self._input_rows(keep)
            if x_rows is None:
                audio = keep[0] if len(keep) == 1 else torch.cat(keep, dim=0)
            else:
                audio = keep[0]
        if audio.dim() != 3 or audio.shape[1] != 2:
            raise ValueError(f"audio must be (items * nb_samples, 2, n); got {tuple(audio.shape)}")
        B = audio.shape[0] * (len(keep) if x_rows is not None else 1)
        n = audio.shape[-1]
        self._packed_fft()
        if n > self.chunk_size:
            raise ValueError(f"work items are at most chunk_size = {self.chunk_size} samples (got {n})")
        if tuple(row_offsets.shape) != (4, B, 2) or row_offsets.dtype != torch.int64:
            raise ValueError(f"row_offsets must be int64 (4, {B}, 2); got {tuple(row_offsets.shape)}")
        wiener = self._native_mode(audio)
        if wiener is not None and out.is_contiguous() and out.dtype == torch.float32 and B % max(1, group) == 0:
            # one C call per pass (xsq_demix_pass): the zero padding of a short item is a slice count, not a copy
            if x_rows is None:                     # (a row table addresses the items where they lie)
                audio = _fp32(audio)
            offs = row_offsets if row_offsets.is_contiguous() else row_offsets.contiguous()
            c = self._native_call(audio.device)
            with torch.cuda.device(c.dev):
                stream = c.main.cuda_stream
                n_pad = max(n, int(self.nsgt.nsgt.sllen / 2) + 1)
                # (no schedule cuts a pass: neither the cap nor ``_plan_sizes`` has a part in it)
                key = ("pass", B, n_pad, wiener, self._handle_key(), c.dev.index)
                nbytes = self.__dict__.setdefault("_nsizes", {}).get(key)
                if nbytes is None:
                    nbytes = self._nsizes[key] = _lib.workspace_bytes("xsq_demix_pass_workspace", c.d, c.model, B, n_pad, wiener)
                ws = self._native_ws(c.dev, stream, "pass", nbytes)
                _lib.call("xsq_demix_pass", c.d, c.model, audio.data_ptr(), x_rows.data_ptr() if x_rows is not None else None, B, n, n_pad,
                          int(group), wiener, out.data_ptr(), offs.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            return
        if x_rows is not None:
            audio = torch.cat(keep, dim=0)
        self._demix_py(out, audio, n, row_offsets, group)

    # -- the native whole-call path ---------------------------------------------------------------------------
    def _native_mode(self, audio: Tensor):
        """None when this call has to take the Python chunk loop (an A/B switch is off its default, a mixed or
        non-stereo model), else the post-filter of the native call: 0 mix-phase, k >= 1 Wiener-EM of k iterations
        (``niter``; 0 on an offline model is mix-phase).  Every entry point comes through here: a realtime model asked for
        ``softmask`` or ``residual`` is refused (``XsqError`` naming the option)."""
        self.xumx_model.wiener_options()
        if audio.dim() != 3 or audio.shape[1] != 2 or audio.device.type != "cuda" or audio.shape[-1] < 1:
            return None
        if not self._native_switches():
            return None
        modes = {bool(b.realtime) for b in self.xumx_model.sliced_umx}
        if len(modes) != 1:
            return None
        return 0 if modes.pop() else self.niter

    def _native_switches(self) -> bool:
        """Every A/B switch stands at its default: the native entry points serve the call."""
        return bool(switch(self, "native") and switch(self, "batch_chunks") and switch(self, "pass_streams") == 1
                    and switch(self, "fuse_whiten") and switch(self, "fuse_phasemix")
                    and switch(self.xumx_model, "wiener_masked") and switch(self.xumx_model, "niter_method") == "auto")

    def _native_ws(self, dev: torch.device, stream_ptr: int, which: str, nbytes: int) -> Tensor:
        """Grow-only workspace of the native path per (device, stream, main | tail | ...)."""
        return self._nws.get(dev, nbytes, stream_ptr, which)

    def _stream_pool(self, dev: torch.device, n: int = 1) -> list:
        """At least ``n`` side streams of ``dev``: pool[0] = the tail's, pool[1:] = extra pass streams."""
        pool = self.__dict__.setdefault("_side_streams", {}).setdefault(dev.index, [])
        while len(pool) < n:
            pool.append(torch.cuda.Stream(device=dev))
        return pool

    def _native_call(self, dev: torch.device) -> _Native:
        """What a native entry point needs before its C calls: the device with an index, the model handle, the demixer, the
        caller's stream and the chunking numbers (``cs``, ``max_stack``, the ``max_item_slices`` cap)."""
        if dev.index is None:
            dev = torch.device("cuda", _lib.device_index(dev))
        return _Native(dev, self.xumx_model._model(dev), self.nsgt.nsgt.nsgt.demixer(dev), torch.cuda.current_stream(dev),
                       int(min(self.chunk_size, 1 << 62)), switch(self, "max_stack"), switch(self, "max_item_slices"))

    def _plan_sizes(self, c: _Native, kind: str, args: tuple, query: str, nout: int):
        """The ``nout`` workspace byte counts of a whole-call shape under the current cap, ``query(d, model, *args, &size...)``:
        asked of the library once per (kind, args, model handle, device, cap) and kept in ``_nsizes``."""
        # the cap is sticky state of the native demixer and part of its plan key: set it on EVERY call, not only on a
        # miss of ``_nsizes`` -- after 0 -> 20 -> 0 a cached shape would otherwise run under the stale cap
        _lib.call("xsq_demixer_set_max_rows", c.d, c.cap)
        key = (kind,) + args + (self._handle_key(), c.dev.index, c.cap)
        sizes = self.__dict__.setdefault("_nsizes", {})
        if key not in sizes:
            outs = [C.c_size_t() for _ in range(nout)]
            _lib.call(query, c.d, c.model, *args, *map(C.byref, outs))
            sizes[key] = outs[0].value if nout == 1 else tuple(o.value for o in outs)
        return sizes[key]

    def _forward_native(self, audio_big: Tensor, wiener: int, slot: Optional[Tensor] = None, gains: Optional[Tensor] = None) -> Tensor:
        """``forward`` as ONE C call (xsq_separator_forward, csrc/demix.hip): the stacked full chunks on the caller's
        stream, the tail chunk beside them on a side stream, the input read and the stems written in place through
        row-offset tables cached per call shape.  Per call the host allocates the result and makes one ctypes call.
        ``gains`` (host fp32 (R, 4)): the R mixes of ``remix`` instead of the stems (xsq_separator_remix, same schedule
        and workspaces)."""
        audio_big = _fp32(audio_big)
        self._packed_fft()
        c = self._native_call(audio_big.device)
        with torch.cuda.device(c.dev):
            nb, N, dev, main = audio_big.shape[0], audio_big.shape[-1], c.dev, c.main
            overlap = switch(self, "overlap_tail")
            side = self._stream_pool(dev)[0] if overlap else main
            sizes = self._plan_sizes(c, "forward", (nb, N, c.cs, c.max_stack, wiener), "xsq_separator_workspace", 2)
            two = overlap and sizes[1] > 0
            ws = self._native_ws(dev, main.cuda_stream, "main", sizes[0] if two else max(sizes))
            wt = self._native_ws(dev, main.cuda_stream, "tail", sizes[1]) if two else None
            out = torch.empty(self._nb_sources() if gains is None else gains.shape[0], nb, 2, N, dtype=torch.float32, device=dev)
            # the result, the two workspaces and the two streams: the arguments all three whole-call signatures share
            shared = (1 if two else 0, out.data_ptr(), ws.data_ptr(), ws.numel(), wt.data_ptr() if two else None, wt.numel() if two else 0,
                      main.cuda_stream, side.cuda_stream if two else main.cuda_stream)
            if gains is not None:
                _lib.call("xsq_separator_remix", c.d, c.model, audio_big.data_ptr(), nb, N, c.cs, c.max_stack, wiener, *shared,
                          gains.data_ptr(), int(gains.shape[0]))
                return out
            name, src = (("xsq_separator_forward", audio_big.data_ptr()) if slot is None
                         else ("xsq_separator_forward_indirect", slot.data_ptr()))
            _lib.call(name, c.d, c.model, src, nb, N, c.cs, c.max_stack, wiener, *shared)
        return out

    def _stacked_chunks(self, nb: int, N: int, cs: int):
        """[(first sample, chunks)] of the stacked passes of the Python chunk loop: the FULL chunks of an N-sample call, at
        most ``max_stack`` (chunk, sample) pairs per pass -- that bounds the workspaces (~1.8 GB per stacked full chunk) and
        keeps BC*S inside one launch for any track length; a single chunk is no stack.  ``batch_chunks = False``: none."""
        full = N // cs if switch(self, "batch_chunks") else 0
        per_pass = max(1, switch(self, "max_stack") // nb)
        stacked, start0 = [], 0
        while full - start0 // cs >= 2 and per_pass >= 2:
            k = min(per_pass, full - start0 // cs)
            stacked.append((start0, k))
            start0 += k * cs
        return stacked

    @torch.no_grad()
    def forward(self, audio_big: Tensor) -> Tensor:
        """(nb_samples, 2, N) fp32 on a ROCm device -> (4, nb_samples, 2, N); (5, ...) with ``residual``, the residual last.
        separator.py:133-232: chunks of chunk_size samples, short chunks zero-padded to sllen/2+1, hard concat.

        The reference walks the chunks one by one; no state crosses the loop, so here all FULL
        chunks of the call are stacked along the batch axis and run as one pass (the Wiener
        window maximum stays per chunk via ``wiener_batch_group``) -- same numbers, a fifth of the
        launches.  By default the whole call is issued by native code (``_forward_native``); the Python
        loop below is the same schedule spelled through the module API and serves the A/B switches
        (``native = False``, ``batch_chunks = False`` for the literal loop, ``fuse_* = False``, ...)."""
        wiener = self._native_mode(audio_big)
        if wiener is not None:
            return self._forward_native(audio_big, wiener)
        nb, N, cs = audio_big.shape[0], audio_big.shape[-1], self.chunk_size
        dev = audio_big.device
        self._packed_fft()
        # every chunk's stems are written straight into their place of the result (the hard concat
        # of separator.py:231 without a copy): packed channel (target, [chunk,] b, c) -> out row
        J = self._nb_sources()
        out = torch.empty(J, nb, 2, N, dtype=torch.float32, device=dev)
        rows = (torch.arange(J, device=dev).view(J, 1, 1, 1) * nb + torch.arange(nb, device=dev).view(1, 1, nb, 1)) * 2 \
            + torch.arange(2, device=dev).view(1, 1, 1, 2)                       # (J, 1, nb, 2) row of `out`

        def rest(first):
            for start in range(first, N, cs):
                audio = audio_big[..., start:min(start + cs, N)]
                self._demix_py(out, audio, audio.shape[-1], rows * N + start)

        stacked = self._stacked_chunks(nb, N, cs)
        if not stacked:
            rest(0)
            return out
        # The remaining chunks (the short tail of the track) are launch-bound -- a dozen kernels of a few
        # hundred workgroups each -- and independent of the stacked passes: they go out FIRST, on a side stream
        # with its own workspaces, and fill in beside the big launches instead of running after them.  The
        # stacked passes themselves are dealt to `pass_streams` streams (default 1: all on the caller's).
        main = torch.cuda.current_stream(dev)
        tail_first = stacked[-1][0] + stacked[-1][1] * cs
        nstreams = max(1, min(switch(self, "pass_streams"), len(stacked)))
        overlap_tail = tail_first < N and switch(self, "overlap_tail")
        pool = self._stream_pool(dev, nstreams)
        used = []
        if overlap_tail:
            pool[0].wait_stream(main)
            used.append(pool[0])
            with torch.cuda.stream(pool[0]):
                rest(tail_first)
        for i, (s0, k) in enumerate(stacked):
            st = main if i % nstreams == 0 else pool[i % nstreams]
            if st is not main and st not in used:
                st.wait_stream(main)
                used.append(st)
            with torch.cuda.stream(st):
                a = audio_big[..., s0:s0 + k * cs].reshape(nb, 2, k, cs).permute(2, 0, 1, 3).reshape(k * nb, 2, cs)
                offs = rows * N + s0 + torch.arange(k, device=dev).view(1, k, 1, 1) * cs   # (J, k, nb, 2)
                self._demix_py(out, a, cs, offs, group=nb)                       # batch = (chunk, b)
        for st in used:
            main.wait_stream(st)
        if not overlap_tail:
            rest(tail_first)
        return out

    @torch.no_grad()
    def remix(self, audio_big: Tensor, gains) -> Tensor:
        """(nb_samples, 2, N) fp32 on a ROCm device -> (R, nb_samples, 2, N): R <= 4 gain-weighted mixes of the stems,
        mix r = sum_t gains[r, t] * forward(audio)[t] -- the slider mix of demixui.py:94-114, remix_signal of
        cadenza/enhance.py:270-290, the target groups of to_dict (separator.py:235-259).  ``gains``: see ``remix_gains``
        (an (R, 4) or (4,) array in ``sources`` order, a {target: gain} dict -- unnamed targets keep 1.0 -- or a list of
        such dicts).  The inverse transform is linear, so the native path runs R inverse transforms per chunk instead of
        four plus a sum (xsq_separator_remix); a target no row weights is never read.  When this call takes the Python
        chunk loop (``_native_mode`` is None: an A/B switch off its default, a mixed model) the result is computed by
        definition, ``einsum("rt,tbcn->rbcn", G, forward(audio))``.  ``softmask`` is honoured; ``residual`` is refused
        (ValueError): a gain row has four columns and the residual is no target."""
        G = remix_gains(gains)
        if self.residual:
            raise ValueError("remix weights the four targets; residual = True adds a fifth stem that no gain column names: "
                             "switch residual off, or mix the five stems of forward yourself")
        if not isinstance(audio_big, Tensor) or audio_big.device.type != "cuda":
            raise ValueError("remix needs the audio on a ROCm device (as forward)")
        wiener = self._native_mode(audio_big)
        if wiener is None:
            est = self.forward(audio_big)
            return torch.einsum("rt,tbcn->rbcn", G.to(device=est.device, dtype=est.dtype), est)
        return self._forward_native(audio_big, wiener, gains=G)

    def _segment_lengths(self, segment: float, overlap: float, sample_rate=None):
        """(chunk_len, ov) of ``forward_overlapped`` in samples; ValueError for what the segment rule cannot use."""
        if sample_rate is None:
            sample_rate = self.__dict__.get("_sr")
            if sample_rate is None:                       # (the buffer lives on the device: read it once)
                sample_rate = self.__dict__["_sr"] = float(self.sample_rate)
        return segment_lengths(sample_rate, segment, overlap, self.chunk_size)

    @torch.no_grad()
    def forward_overlapped(self, audio_big: Tensor, segment: float = 10.0, overlap: float = 0.1) -> Tensor:
        """(nb_samples, 2, N) fp32 on a ROCm device -> (4, nb_samples, 2, N) ((5, ...) with ``residual``): ``forward`` over segments that overlap and are
        cross-faded, ``separate_sources`` of the reference's Cadenza caller (cadenza/enhance.py:35-99) instead of the hard
        concat of separator.py:231.  ``segment`` seconds per hop, ``overlap`` in [0, 1) of a second: with
        chunk_len = int(sr * segment * (1 + overlap)) and ov = int(overlap * sr), segment k starts at k * chunk_len - ov
        (0 for k = 0), ends at (k + 1) * chunk_len and fades linearly (torchaudio ``Fade``) over the ov samples it shares
        with each neighbour; ``segments`` lists them.  Two departures from the reference: a segment without
        a successor does not fade out, and the first hop is taken in integers.
        By default ONE native call (xsq_separator_forward_segments: equal-length segments stacked into passes, read in
        place, blended by one xsq_crossfade_place launch per pass).  When ``_native_mode`` is None (an A/B switch off its
        default, a mixed model) the definition is computed: ``forward`` per segment, faded and added with torch."""
        if not isinstance(audio_big, Tensor) or audio_big.dim() != 3:
            raise ValueError("forward_overlapped needs (nb_samples, 2, N) audio (as forward)")
        chunk_len, ov = self._segment_lengths(segment, overlap)
        if audio_big.shape[-1] <= ov:
            raise ValueError(f"a track of {audio_big.shape[-1]} samples is not longer than the overlap of {ov}: no segment exists")
        wiener = self._native_mode(audio_big)
        if wiener is None:
            return overlapped_loop(self.forward, audio_big, chunk_len, ov)
        audio_big = _fp32(audio_big)
        self._packed_fft()
        c = self._native_call(audio_big.device)
        with torch.cuda.device(c.dev):
            nb, N, stream = audio_big.shape[0], audio_big.shape[-1], c.main.cuda_stream
            args = (nb, N, c.cs, chunk_len, ov, c.max_stack, wiener)
            ws = self._native_ws(c.dev, stream, "main", self._plan_sizes(c, "segments", args, "xsq_separator_segments_workspace", 1))
            out = torch.empty(self._nb_sources(), nb, 2, N, dtype=torch.float32, device=c.dev)
            _lib.call("xsq_separator_forward_segments", c.d, c.model, audio_big.data_ptr(), *args, out.data_ptr(), ws.data_ptr(),
                      ws.numel(), stream)
        return out

    def stream(self, nb_samples: int = 1, hop_slices: int = 1) -> "StreamSession":
        """A stateful session that demixes audio arriving in blocks: ``feed`` returns the samples that became final, ``flush``
        the rest, and the concatenation is ``forward`` of the whole signal by a separator whose ``chunk_size`` holds it -- a
        stream has no chunk joints.  Every ``hop_slices`` blocks of sllen / 2 samples one step runs, as soon as
        the audio 2 * sllen samples past the first of them has arrived (``latency_samples``).  Mix-phase models only: the
        realtime model, or the offline stack with ``niter = 0`` / without Wiener; ``XsqError`` naming the reason for Wiener-EM
        (its statistics span 5000-frame windows from the start of a chunk), ``softmask``, ``residual``, mixed block modes and
        ``hop_slices < 1``."""
        return StreamSession(self, nb_samples, hop_slices)

    @torch.no_grad()
    def forward_aggregate(self, audio_big: Tensor, aggregate_dict: dict) -> dict:
        """``to_dict(forward(audio), aggregate_dict)`` (separator.py:235-259) through ``remix`` with 0/1 gain rows: one
        inverse transform per group instead of four.  At most four groups."""
        names, G = aggregate_gains(aggregate_dict)
        out = self.remix(audio_big, G)
        return {name: out[r] for r, name in enumerate(names)}

    @staticmethod
    def to_dict(estimates: Tensor, aggregate_dict: Optional[dict] = None) -> dict:
        """separator.py:234-259.  Five estimates (``residual``) add the key "residual"."""
        estimates_dict = {target: estimates[k] for k, target in enumerate(Separator.sources)}
        if len(estimates) == 5:
            estimates_dict["residual"] = estimates[4]
        if aggregate_dict is not None:
            new_estimates = {}
            for key in aggregate_dict:
                new_estimates[key] = torch.tensor(0.0)
                for target in aggregate_dict[key]:
                    new_estimates[key] = new_estimates[key] + estimates_dict[target]
            estimates_dict = new_estimates
        return estimates_dict


def segment_lengths(sample_rate, segment: float, overlap: float, chunk_size: Optional[int] = None):
    """(chunk_len, ov) in samples of the overlapped segments (cadenza/enhance.py:75-78, the overlap in integers).
    ValueError for segment <= 0, overlap outside [0, 1), ov >= chunk_len and a segment longer than ``chunk_size``."""
    segment, overlap = float(segment), float(overlap)
    if not segment > 0 or segment == float("inf"):
        raise ValueError(f"segment must be a positive number of seconds (got {segment})")
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"overlap must be in [0, 1) (got {overlap})")
    chunk_len = int(sample_rate * segment * (1 + overlap))
    ov = int(overlap * sample_rate)
    if chunk_len < 1 or ov >= chunk_len:
        raise ValueError(f"segment = {segment} s gives {chunk_len} samples per hop against an overlap of {ov}: too short")
    if chunk_size is not None and chunk_len + ov > chunk_size:
        raise ValueError(f"a segment of {chunk_len} + {ov} samples is longer than chunk_size = {chunk_size}")
    return chunk_len, ov


def segments(N: int, chunk_len: int, ov: int):
    """[(start, samples, fade_in, fade_out)] of the overlapped segments of an N-sample track (xsq_segment_schedule: host
    arithmetic, the one statement of the rule that the native call, the fallback loop and the tests share)."""
    import numpy as np
    buf = np.zeros((max(1, N // max(1, chunk_len) + 2), 4), dtype=np.int64)
    n = _lib.lib.xsq_segment_schedule(int(N), int(chunk_len), int(ov), buf.ctypes.data, len(buf))
    if n < 0 or n > len(buf):
        raise ValueError(f"xsq_segment_schedule({N}, {chunk_len}, {ov}): {_lib.last_error() if n < 0 else n}")
    return [tuple(r) for r in buf[:n].tolist()]


def fade_weights(ov: int, device=None):
    """(w_in, w_out) of torchaudio's linear Fade over ov >= 1 samples, fp32: i / (ov - 1) and (ov - 1 - i) / (ov - 1), one
    rounding each (the quotients the crossfade kernel forms); ov == 1: [0] and [1]."""
    if ov == 1:
        return torch.zeros(1, device=device), torch.ones(1, device=device)
    i = torch.arange(ov, dtype=torch.float32)
    return (i / float(ov - 1)).to(device), (i.flip(0) / float(ov - 1)).to(device)


def overlapped_loop(forward, audio: Tensor, chunk_len: int, ov: int) -> Tensor:
    """The definition of ``Separator.forward_overlapped``: ``forward`` (any callable (nb, ch, n) -> (4, nb, ch, n)) per
    segment, each faded and added into the result in segment order.  The tail of a segment is stored as w_out * a and the
    head of the next added as w_in * b: products and sum rounded one by one, as the native call does."""
    nb, ch, N = audio.shape
    segs = segments(N, chunk_len, ov)
    if not segs:
        raise ValueError(f"a track of {N} samples is not longer than the overlap of {ov}: no segment exists")
    out = None
    for start, n, fi, fo in segs:
        est = forward(audio[..., start:start + n])
        if out is None:
            out = torch.empty((*est.shape[:-1], N), dtype=est.dtype, device=est.device)
            w_in, w_out = fade_weights(ov, est.device) if ov else (None, None)
        if fi:
            out[..., start:start + fi] += w_in * est[..., :fi]
        out[..., start + fi:start + n - fo] = est[..., fi:n - fo]
        if fo:
            out[..., start + n - fo:start + n] = w_out * est[..., n - fo:]
    return out


def stream_steps(N: int, L: int, hop_slices: int, back: int, ahead: int = STREAM_AHEAD):
    """[(first block, blocks, first slice inverted, first slice of the window, last slice of the window, samples fed when it
    fires)] of a stream of N samples in all (xsq_stream_schedule: host arithmetic, the one statement of the rule that the
    native session, ``streamed_loop`` and the tests share).  Block k = samples [k L / 2, (k + 1) L / 2)."""
    import numpy as np
    if hop_slices < 1:
        raise ValueError(f"hop_slices must be >= 1 (got {hop_slices})")
    buf = np.zeros((max(1, 2 * N // max(1, L * hop_slices) + 2), 6), dtype=np.int64)
    n = _lib.lib.xsq_stream_schedule(int(N), int(L), int(hop_slices), int(back), int(ahead), buf.ctypes.data, len(buf))
    if n < 0 or n > len(buf):
        raise ValueError(f"xsq_stream_schedule({N}, {L}, {hop_slices}, {back}, {ahead}): {_lib.last_error() if n < 0 else n}")
    return [tuple(r) for r in buf[:n].tolist()]


def stream_trigger(step: int, L: int, hop_slices: int, ahead: int = STREAM_AHEAD) -> int:
    """Samples that must have been fed before step ``step`` of an open stream runs: its last window slice is complete."""
    return (2 * ((step + 1) * hop_slices + ahead) + 2) * (L // 4)


def _loop_span(b0: int, w1: int, h: int, back: int, N: Optional[int]):
    """(t0, t1) of the sub-signal whose ``forward`` gives the blocks from b0 on their full context: one slice more than the window
    on each side, because a plain ``forward`` cuts its first and its last slice against zeros.  The window starts ``back`` slices
    behind slice b0, whose second half opens block b0."""
    t0 = 2 * h * max(0, max(0, b0 - back) - 1)
    t1 = (2 * w1 + 2) * h
    return t0, (t1 if N is None else min(N, t1))


def streamed_loop(forward, audio: Tensor, L: int, hop_slices: int, back: int, ahead: int = STREAM_AHEAD) -> Tensor:
    """The schedule of a streaming session spelled through any ``forward`` (a callable (nb, ch, n) -> (J, nb, ch, n)): one call
    per step of ``stream_steps`` on the sub-signal that gives the step's blocks their context, the blocks copied out of its
    result.  With ``back`` / ``ahead`` at least the dependency window of the model behind ``forward`` the result is
    ``forward(audio)``; one slice short it is not (tests/test_stream_cpu.py holds both)."""
    nb, ch, N = audio.shape
    if N < 1:
        raise ValueError("streamed_loop: no samples")
    h = L // 4
    out = None
    for b0, blocks, _first, _w0, w1, _trigger in stream_steps(N, L, hop_slices, back, ahead):
        t0, t1 = _loop_span(b0, w1, h, back, N)
        est = forward(audio[..., t0:t1])
        if out is None:
            out = torch.empty((*est.shape[:-1], N), dtype=est.dtype, device=est.device)
        lo, n = b0 * 2 * h, min(blocks * 2 * h, N - b0 * 2 * h)
        out[..., lo:lo + n] = est[..., lo - t0:lo - t0 + n]
    return out


class StreamGrid:
    """The host bookkeeping of a streaming session, no device: which steps of the absolute block grid a run of ``feed`` calls
    and the final ``flush`` fire.  The steps depend on the samples fed in all and on ``hop_slices``, never on the partition."""

    def __init__(self, L: int, hop_slices: int, back: int, ahead: int = STREAM_AHEAD):
        self.L, self.hop_slices, self.back, self.ahead = int(L), int(hop_slices), int(back), int(ahead)
        self.samples_in = self.steps = 0

    def trigger(self) -> int:
        return stream_trigger(self.steps, self.L, self.hop_slices, self.ahead)

    def feed(self, n: int):
        """[(count, step)]: ``count`` more samples enter, then step ``step`` runs (None: none does -- the last entry at most)."""
        events = []
        while n > 0:
            count = min(n, self.trigger() - self.samples_in)
            self.samples_in, n = self.samples_in + count, n - count
            fires = self.samples_in == self.trigger()
            events.append((count, self.steps if fires else None))
            self.steps += int(fires)
        return events

    def flush(self):
        """The ``stream_steps`` rows of the steps that only the end of the stream releases."""
        steps = stream_steps(self.samples_in, self.L, self.hop_slices, self.back, self.ahead)[self.steps:]
        self.steps += len(steps)
        return steps


class StreamSession:
    """``Separator.stream``: see there.  ``feed`` / ``flush`` return (4, nb_samples, 2, k); every launch goes to the caller's
    current stream and nothing waits on the host.  By default one native call per step (xsq_stream_step) on device state that
    does not grow: an audio ring and the carried half slice per output channel.  When an A/B switch is off its default
    (``native = False``, ...) the steps are ``streamed_loop``'s: ``forward`` on a kept tail of the input."""

    def __init__(self, separator: Separator, nb_samples: int = 1, hop_slices: int = 1):
        model = separator.xumx_model
        if int(hop_slices) < 1:
            raise _lib.XsqError(f"stream: hop_slices must be >= 1 (got {hop_slices})")
        if int(nb_samples) < 1:
            raise _lib.XsqError(f"stream: nb_samples must be >= 1 (got {nb_samples})")
        modes = {bool(b.realtime) for b in model.sliced_umx}
        causal = {bool(b.causal) for b in model.sliced_umx}
        if len(modes) != 1 or len(causal) != 1:
            raise _lib.XsqError("stream: mixed per-block modes (some mix-phase, some Wiener; some causal, some not) are not supported")
        if separator.softmask or separator.residual:
            which = " and ".join(n for n in ("softmask", "residual") if getattr(separator, n))
            raise _lib.XsqError(f"stream: {which} belongs to the Wiener post-filter, which cannot stream; a session is mix-phase")
        if not modes.pop() and separator.niter >= 1:
            raise _lib.XsqError(f"stream: Wiener-EM (niter = {separator.niter} on an offline model) cannot stream: its statistics span "
                                "5000-frame windows counted from the start of a chunk and the window maximum; use the realtime model, "
                                "niter = 0 or wiener = False")
        if getattr(separator, "dc_twins", False):
            raise _lib.XsqError("stream: a plan with bands across DC (dc_twins = True) cannot stream: the mirrored synthesis turns with the "
                                "parity of a slice's index in the whole stream, which the carried step does not keep")
        if getattr(separator, "long_bands", False):
            raise _lib.XsqError("stream: a plan with bands on the FFT band engine (long_bands = True) cannot stream: the carried step has "
                                "not been taken through blocks of thousands of frames")
        self.separator = separator
        self.nb_samples, self.hop_slices = int(nb_samples), int(hop_slices)
        self.back, self.ahead = STREAM_BACK[causal.pop()], STREAM_AHEAD
        self.L = int(separator.nsgt.nsgt.sllen)
        self.h = self.L // 4
        self._grid = StreamGrid(self.L, self.hop_slices, self.back, self.ahead)
        self.samples_out = 0
        self._closed = False
        self._native = separator._native_switches()
        self._handle = self._state = self._hist = None
        self._hist0 = 0
        self._ws_bytes = {}
        if self._native:
            dev = torch.device(separator.device)
            if dev.type != "cuda":
                raise _lib.XsqError(f"stream: a session lives on a ROCm device (the separator's is '{dev}')")
            c = separator._native_call(dev)
            handle = C.c_void_p()
            _lib.call("xsq_stream_create", C.byref(handle), c.d, c.model, self.nb_samples, self.hop_slices, self.back, self.ahead)
            self._handle = handle
            self._finalizer = weakref.finalize(self, _lib.lib.xsq_stream_destroy, handle)
            with torch.cuda.device(c.dev):
                self._state = torch.empty(int(_lib.lib.xsq_stream_state_bytes(handle)), dtype=torch.uint8, device=c.dev)
            self._dev = c.dev

    latency_samples = property(lambda self: (2 * self.ahead + 4) * self.h,
                               doc="samples from the first of a block to the one that releases it at hop_slices = 1: 2 * sllen")

    samples_in = property(lambda self: self._grid.samples_in, doc="samples fed so far")

    @property
    def state_bytes(self) -> int:
        """Device memory the session holds between calls (the shared, grow-only step workspace of the separator is not its own)."""
        if self._native:
            return int(self._state.numel())
        return 0 if self._hist is None else int(self._hist.numel() * self._hist.element_size())

    def _empty(self, device, k: int) -> Tensor:
        return torch.empty(4, self.nb_samples, 2, k, dtype=torch.float32, device=device)

    def _check(self, block: Tensor) -> Tensor:
        if self._closed:
            raise _lib.XsqError("stream: the session was flushed; open a new one with Separator.stream()")
        if not isinstance(block, Tensor) or block.dim() != 3 or tuple(block.shape[:2]) != (self.nb_samples, 2):
            raise ValueError(f"feed wants ({self.nb_samples}, 2, n) audio; got {tuple(getattr(block, 'shape', ()))}")
        if block.device.type != "cuda":
            raise ValueError("feed needs the audio on a ROCm device (as forward)")
        # a view along the samples of a longer (nb_samples, 2, N) tensor is read where it lies: rows one row stride apart
        if block.dtype == torch.float32 and block.shape[-1] > 0 and block.stride(-1) == 1 and block.stride(1) >= block.shape[-1] \
                and (self.nb_samples == 1 or block.stride(0) == 2 * block.stride(1)):
            return block
        return _fp32(block)

    def _step_native(self, c: _Native, ws: Tensor, total: int, out: Tensor, col: int, length: int, new=(None, 0, 0)):
        """``new`` = (address, row stride, count) of the samples that release the step: they ride on its first kernel."""
        _lib.call("xsq_stream_step", self._handle, c.model, self._state.data_ptr(), *new, total, out.data_ptr() + 4 * col, out.shape[-1],
                  length, ws.data_ptr(), ws.numel(), c.main.cuda_stream)

    def _native_setup(self):
        sep = self.separator
        c = sep._native_call(self._dev)
        key = sep._handle_key()
        if key not in self._ws_bytes:
            self._ws_bytes = {key: _lib.workspace_bytes("xsq_stream_workspace", self._handle, c.model)}
        return c, sep._native_ws(c.dev, c.main.cuda_stream, "stream", self._ws_bytes[key])

    def _step_py(self, total: Optional[int], b0: int, blocks: int, w1: int, out: Tensor, col: int, length: int):
        """One step of ``streamed_loop`` on the kept tail of the input, which then drops what no later step reads."""
        t0, t1 = _loop_span(b0, w1, self.h, self.back, total)
        est = self.separator.forward(self._hist[..., t0 - self._hist0:t1 - self._hist0])
        lo = b0 * 2 * self.h - t0
        out[..., col:col + length] = est[..., lo:lo + length]
        keep = _loop_span(b0 + self.hop_slices, 0, self.h, self.back, None)[0]
        self._hist, self._hist0 = self._hist[..., keep - self._hist0:], keep

    @torch.no_grad()
    def feed(self, block: Tensor) -> Tensor:
        """``block`` (nb_samples, 2, n) fp32 on the device, any n >= 0 -> (4, nb_samples, 2, k): the samples that became final
        with it, k a multiple of hop_slices * sllen / 2 (possibly 0)."""
        block = self._check(block)
        n, per = block.shape[-1], 2 * self.h * self.hop_slices
        events = self._grid.feed(n)
        fired = [step for _, step in events if step is not None]
        out = self._empty(block.device, len(fired) * per)
        if n == 0:
            return out
        if not self._native:
            self._hist = block.clone() if self._hist is None else torch.cat([self._hist, block], dim=-1)
            for i, step in enumerate(fired):
                b0 = step * self.hop_slices
                self._step_py(None, b0, self.hop_slices, b0 + self.hop_slices + self.ahead, out, i * per, per)
            self.samples_out += len(fired) * per
            return out
        self.separator._packed_fft()
        c, ws = self._native_setup()
        with torch.cuda.device(c.dev):
            pos = col = 0
            for count, step in events:
                if step is not None:
                    self._step_native(c, ws, -1, out, col, per, new=(block.data_ptr() + 4 * pos, block.stride(1), count))
                    col += per
                else:
                    _lib.call("xsq_stream_push", self._handle, self._state.data_ptr(), block.data_ptr() + 4 * pos, block.stride(1), count,
                              c.main.cuda_stream)
                pos += count
        self.samples_out += col
        return out

    @torch.no_grad()
    def flush(self) -> Tensor:
        """The rest: the blocks no later sample can change any more, the last one cut at the samples fed.  Closes the session."""
        if self._closed:
            raise _lib.XsqError("stream: the session was flushed already")
        self._closed = True
        N = self.samples_in
        dev = self._dev if self._native else (self._hist.device if self._hist is not None else torch.device(self.separator.device))
        out = self._empty(dev, N - self.samples_out)
        steps = self._grid.flush()
        if not steps:
            return out
        if self._native:
            self.separator._packed_fft()
            c, ws = self._native_setup()
        col = 0
        for b0, blocks, _first, _w0, w1, _trigger in steps:
            length = min(blocks * 2 * self.h, N - b0 * 2 * self.h)
            if self._native:
                with torch.cuda.device(c.dev):
                    self._step_native(c, ws, N, out, col, length)
            else:
                self._step_py(N, b0, blocks, w1, out, col, length)
            col += length
        self.samples_out += col
        assert self.samples_out == N, (self.samples_out, N)
        self._hist = None
        return out


def _gain_row(d: dict) -> list:
    unknown = [k for k in d if k not in Separator.sources]
    if unknown:
        raise ValueError(f"unknown target(s) {unknown}; the targets are {Separator.sources}")
    return [float(d.get(t, 1.0)) for t in Separator.sources]


def remix_gains(gains) -> Tensor:
    """Gain matrix (R, 4) fp32 on the host for ``Separator.remix``, targets in ``Separator.sources`` order, from
    - an (R, 4) or (4,) tensor / array / nested list of numbers;
    - a {target: gain} dict: one row, targets not named keep gain 1.0 ({"vocals": 0} is karaoke);
    - a list of such dicts: one row each.
    ValueError for unknown targets, a shape other than (R, 4) with 1 <= R <= 4, and non-finite gains."""
    if isinstance(gains, dict):
        rows = [_gain_row(gains)]
    elif isinstance(gains, (list, tuple)) and len(gains) > 0 and all(isinstance(g, dict) for g in gains):
        rows = [_gain_row(g) for g in gains]
    elif isinstance(gains, (list, tuple)) and any(isinstance(g, dict) for g in gains):
        raise ValueError("a list of gains is all dicts or all numbers")
    else:
        rows = gains
    try:
        G = torch.as_tensor(rows.detach().cpu() if isinstance(rows, Tensor) else rows, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"gains must be an (R, 4) array, a {{target: gain}} dict or a list of dicts ({e})") from None
    if G.dim() == 1:
        G = G[None]
    if G.dim() != 2 or G.shape[1] != 4 or not 1 <= G.shape[0] <= 4:
        raise ValueError(f"gains must be (R, 4) with 1 <= R <= 4, targets {Separator.sources}; got {tuple(G.shape)}")
    if not bool(torch.isfinite(G).all()):
        raise ValueError("gains must be finite")
    return G.contiguous()


def aggregate_gains(aggregate_dict: dict):
    """(group names, (R, 4) 0/1 gain matrix) of a to_dict aggregate_dict ({group: [targets]}, at most four groups)."""
    if not isinstance(aggregate_dict, dict) or not 1 <= len(aggregate_dict) <= 4:
        raise ValueError("aggregate_dict must be a dict of 1 to 4 groups {name: [targets]}")
    names, rows = list(aggregate_dict), []
    for name in names:
        row = [0.0] * 4
        for t in aggregate_dict[name]:
            if t not in Separator.sources:
                raise ValueError(f"unknown target {t!r} in group {name!r}; the targets are {Separator.sources}")
            row[Separator.sources.index(t)] += 1.0        # a target named twice counts twice, as in to_dict
        rows.append(row)
    return names, torch.tensor(rows, dtype=torch.float32)


def build_models(fscale: str = "bark", fbins: int = 262, fmin: float = 32.9, sample_rate: float = 44100.0,
                 seq_dur: float = 2.0, realtime: bool = False, device="cuda", state=None,
                 strict: bool = True, dc_twins: bool = False, long_bands: bool = False, fgamma: float = 15.0):
    """Plan + filterbanks + Unmix from explicit config (what load_target_models does after
    reading the JSON, separator.py:321-356).  ``dc_twins``, ``long_bands``, ``fgamma``: see ``plan.build_plan``."""
    nsgt_base = NSGTBase(fscale, fbins, fmin, fgamma=fgamma, fs=sample_rate, device=device, dc_twins=dc_twins, long_bands=long_bands)
    jagged_slicq, _ = nsgt_base.predict_input_size(1, 2, seq_dur)
    cnorm = ComplexNorm()
    nsgt, insgt = make_filterbanks(nsgt_base, sample_rate)
    xumx_model = Unmix(cnorm(jagged_slicq), realtime=realtime, weights_follow=state is not None and strict)
    if state is not None:
        # the reference loads with strict=False and silently drops mismatches (quirk A7); be strict
        xumx_model.load_state_dict(state, strict=strict)
    xumx_model.freeze()
    return xumx_model, (nsgt, insgt, cnorm), sample_rate


def load_target_models(model_path: str, runtime_backend: str = _ACCELERATED, realtime: bool = False,
                       device="cuda", dc_twins: bool = False, long_bands: bool = False, fgamma: float = 15.0):
    """separator.py:262-387 for the accelerated backend: <model_path>/xumx_slicq_v2.json
    (args.sample_rate, fscale, fbins, fmin, seq_dur, realtime; fgamma where the key is there, else the keyword) + xumx_slicq_v2.pth."""
    if runtime_backend != _ACCELERATED:
        raise ValueError(f"unsupported runtime backend: {runtime_backend}")
    if model_path is None:
        raise ValueError("model_path is required: there is no network to download the pretrained model from")
    model_path = Path(model_path).expanduser()
    json_path = Path(model_path, "xumx_slicq_v2.json")
    assert model_path.exists() and json_path.exists()
    with open(json_path, "r") as stream:
        results = json.load(stream)
    pth = Path(model_path, "xumx_slicq_v2.pth")
    if pth.stat().st_size < 4096:
        raise RuntimeError(f"{pth} is a Git-LFS pointer, not a checkpoint; fetch the real weights or use "
                           "seeded_separator() for synthetic ones")
    state = torch.load(pth, map_location="cpu")
    args = results["args"]
    return build_models(args["fscale"], args["fbins"], args["fmin"], args["sample_rate"], args["seq_dur"],
                        realtime=args["realtime"], device=device, state=state, dc_twins=dc_twins, long_bands=long_bands,
                        fgamma=float(args.get("fgamma", fgamma)))


def seeded_separator(realtime: bool = False, wiener: Optional[bool] = None, seed: int = 1234,
                     device="cuda", chunk_size: int = 2621440, niter: Optional[int] = None, softmask: Optional[bool] = None,
                     residual: Optional[bool] = None, dc_twins: bool = False, long_bands: bool = False, fgamma: float = 15.0,
                     **cfg) -> Separator:
    """Separator with the seeded synthetic weights (no checkpoint exists offline).  ``dc_twins``, ``long_bands``, ``fgamma``: see
    ``plan.build_plan``.
    ``wiener`` overrides the post-filter: None follows the reference (offline -> Wiener-EM,
    realtime -> mix-phase); False on the offline stack is BASELINE config 2."""
    xumx_model, encoder, sr = build_models(realtime=realtime, device=device, dc_twins=dc_twins, long_bands=long_bands, fgamma=fgamma, **cfg)
    xumx_model.load_state_dict(seeded_state_dict(xumx_model.table.shapes, seed=seed), strict=True)
    if wiener is not None:
        for blk in xumx_model.sliced_umx:      # the flag the reference reads at model.py:264
            blk.realtime = not wiener
    sep = Separator(xumx_model=xumx_model, encoder=encoder, sample_rate=sr, chunk_size=chunk_size,
                    device=device, quiet=True).to(device)
    sep.freeze()
    _set_wiener_options(sep, niter, softmask, residual)
    return sep
