"""Drop-in mirrors of /root/reference/xumx_slicq_v2/transforms.py on top of the
HIP library: NSGTBase, NSGT_SL, INSGT_SL, ComplexNorm, make_filterbanks.

Same names, argument meaning and error behaviour as the reference.  The
arithmetic is in csrc/slicqt.hip; these classes only own device memory
(PyTorch allocations) and hand pointers across the C ABI.  There is no CPU
path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from .arena import BlockTable
from .plan import SliCQPlan, build_plan


def make_filterbanks(nsgt_base, sample_rate=44100.0):
    """transforms.py:11-18."""
    if sample_rate != 44100.0:
        raise ValueError("i was lazy and harcoded a lot of 44100.0, forgive me")
    return NSGT_SL(nsgt_base), INSGT_SL(nsgt_base)


# The A/B switches of a plan handle: switch -> (its setter in the library, default).  ``SliCQEngine`` keeps each as ``_<switch>``.
_PLAN_SWITCHES = {
    "fft_backend": ("xsq_plan_set_fft_backend", 0),
    "band_radix4": ("xsq_plan_set_band_radix4", True),
    # measured (r02c-e): synthesising the short bands inside the inverse slice FFT kernel is 0.03-0.05 ms SLOWER per
    # 240 s track than the dense GEMM + workspace round trip it replaces (the kernel is bound by its serial chain of
    # memory / LDS round trips, and the in-kernel stage adds three) -> off by default; XSQ_SHORT_INLINE=1 / set_short_inline
    "short_inline": ("xsq_plan_set_short_inline", False),
    "packed_fft": ("xsq_plan_set_packed_fft", False),        # see set_packed_fft
}


class SliCQEngine:
    """Device-side plan handle (the role NSGT_sliced plays in the reference,
    nsgt/slicq.py:70-230).  One handle per device, created on first use."""

    def __init__(self, plan: SliCQPlan):
        self.plan = plan
        self.sl_len = plan.L
        self.tr_area = plan.tr
        self.fs = plan.fs
        self.ncoefs = plan.ncoefs
        self.fbins_actual = plan.nbands
        self.table = BlockTable(plan.block_shapes())
        self._handles = {}
        self._ws = _lib.Scratch()
        for switch, (_, default) in _PLAN_SWITCHES.items():
            setattr(self, "_" + switch, default)
        import os
        self._short_inline = os.environ.get("XSQ_SHORT_INLINE", "0") != "0"

    scratch = property(lambda self: self._ws, doc="the pool of this engine's workspaces (``_lib.Scratch``)")

    def _apply(self, h):
        """Sets the four switches of plan handle ``h`` to this engine's values."""
        for switch, (setter, _) in _PLAN_SWITCHES.items():
            _lib.call(setter, h, int(getattr(self, "_" + switch)))

    def _set(self, switch: str, value):
        """Every live handle first, the engine's own value after: one the library refuses (``XsqError``) is not kept."""
        for h in self._handles.values():
            _lib.call(_PLAN_SWITCHES[switch][0], h, int(value))
        setattr(self, "_" + switch, value)

    def set_fft_backend(self, backend: int):
        """0 = hand-written LDS slice FFT when the plan allows it (default), 1 = rocFFT."""
        self._set("fft_backend", int(backend))

    def set_band_radix4(self, on: bool):
        """True (default): long bands on the radix-4 DFT kernel; False: every band on the dense GEMM."""
        self._set("band_radix4", bool(on))

    def set_packed_fft(self, on: bool):
        """True: the hand-written slice FFT runs its butterflies on packed-fp32 vector instructions (half the vector
        instructions, bitwise the same results).  Diagnostic builds only (csrc/Makefile PACKED_FFT=1): the product library
        refuses (``XsqError``) -- a packed-fp32 transform next to split-bf16 MFMA waves of another stream returned wrong
        values on MI355X and it measured no faster."""
        if bool(on) != self._packed_fft:
            self._set("packed_fft", bool(on))

    def set_short_inline(self, on: bool):
        """False (default): bands with Lg < 24 on the dense GEMM with a round trip through the workspace; True: the inverse
        transform synthesises them inside the slice-FFT kernel (A/B switch, same results to fp32 rounding; measured slower)."""
        self._set("short_inline", bool(on))

    # -- handle management ---------------------------------------------------
    def handle(self, device: torch.device):
        if device.type != "cuda":
            raise _lib.XsqError(
                f"the sliCQT runs on a ROCm device only (got a tensor on '{device}'); there is no CPU fallback")
        idx = _lib.device_index(device)
        h = self._handles.get(idx)
        if h is None:
            p = self.plan
            h = C.c_void_p()
            with torch.cuda.device(idx):
                # a plan built with dc_twins=True: the library derives the table of the mirrored synthesis from Lg, c and gd
                args = (C.byref(h), p.L, p.tr, p.nbands, p.Lg.ctypes.data, p.c.ctypes.data, p.g.ctypes.data, p.gd.ctypes.data, p.tw.ctypes.data)
                if p.long_bands:                         # the bands above 320 on the FFT band engine
                    _lib.call("xsq_plan_create_flags", *args, _lib.PLAN_LONG_BANDS | (_lib.PLAN_TWINS if p.dc_twins else 0))
                else:
                    _lib.call("xsq_plan_create_twins" if p.dc_twins else "xsq_plan_create", *args)
            self._apply(h)
            self._handles[idx] = h
        return h

    def demixer(self, device: torch.device):
        """The native whole-call handle of this plan on ``device`` (xsq_demixer: cached row-offset tables of the call
        shapes + the fork / join events of the tail stream); what ``Separator.forward`` issues a track through."""
        idx = _lib.device_index(device)
        d = self.__dict__.setdefault("_demixers", {}).get(idx)
        if d is None:
            h = self.handle(device)
            out = C.c_void_p()
            with torch.cuda.device(idx):
                _lib.call("xsq_demixer_create", C.byref(out), h)
            d = self._demixers[idx] = out
        return d

    def workspace(self, device: torch.device, nbytes: int) -> Tensor:
        """This engine's grow-only scratch buffer of the current stream on ``device`` (``_lib.Scratch``: calls issued on
        different streams may overlap -- Separator.forward runs the tail chunk beside the stacked pass)."""
        return self._ws.get(device, nbytes)

    def _scratch(self, query: str, device, h, BC: int, extent: int, *more, least: int = 1) -> Tensor:
        """The workspace ``query(h, BC, extent, *more)`` asks for, ``extent`` the samples or slices per channel.  The
        transforms' queries refuse a shape without a message (they set one only where rocFFT refuses a plan), so the shape
        is named here."""
        why = None if BC > 0 and extent >= least else f"{BC} channels of {extent}: needs at least 1 of {least}"
        return self.workspace(device, _lib.workspace_bytes(query, h, BC, extent, *more, why=why))

    def close(self):
        """Frees the device side now -- demixers, plan handles, workspaces -- after the work queued on their devices has ended.
        The engine stays usable: the next call builds new handles.  (A parameter search drops a plan per draw.)"""
        for idx in set(self._handles) | {k[0] for k in self._ws}:
            torch.cuda.synchronize(idx)
        for d in self.__dict__.pop("_demixers", {}).values():
            _lib.lib.xsq_demixer_destroy(d)
        for h in self._handles.values():
            _lib.lib.xsq_plan_destroy(h)
        self._handles.clear()
        self._ws.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __deepcopy__(self, memo):
        """The device plan handles stay with the original (a copied raw handle would be destroyed twice) and the copy of a
        workspace pool is empty; the copy creates its own on first use."""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k in ("_handles", "_demixers") else copy.deepcopy(v, memo)
        return new

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_handles"] = {}
        st.pop("_demixers", None)
        return st

    # -- transforms --------------------------------------------------------------
    def forward(self, x: Tensor, whiten=None):
        """x (*lead, n) fp32 on a ROCm device -> (arena, lead, S).  ``whiten`` = (xin device pointer, mean pointer,
        scale pointer, split flag) from ``Unmix.whitening_target``: the analysis kernels also write the CDAE's
        whitened magnitude there (xsq_slicqt_forward_xin)."""
        if x.dtype != torch.float32:
            x = x.float()
        lead = tuple(x.shape[:-1])
        n = x.shape[-1]
        xb = x.contiguous().view(-1, n)
        BC = xb.shape[0]
        h = self.handle(x.device)
        with torch.cuda.device(x.device):
            S = self.plan.num_slices(n)
            arena = torch.empty(self.table.numel(BC, S), dtype=torch.float32, device=x.device)
            ws = self._scratch("xsq_slicqt_forward_workspace", x.device, h, BC, n)
            if whiten is None:
                _lib.call("xsq_slicqt_forward", h, xb.data_ptr(), BC, n, arena.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
            else:
                xin, mean, scale, split = whiten
                _lib.call("xsq_slicqt_forward_xin", h, xb.data_ptr(), BC, n, arena.data_ptr(), xin, mean, scale, int(split), ws.data_ptr(),
                          ws.numel(), _lib.stream_ptr())
        return arena, lead, S

    def backward(self, arena: Tensor, BC: int, S: int, length: int, out: Tensor = None,
                 row_offsets: Tensor = None) -> Tensor:
        """arena for BC channels, S slices -> (BC, length) fp32.  `arena` is left untouched.
        With ``out`` + ``row_offsets`` (device int64[BC], element offsets into ``out``) packed
        channel r lands at out.view(-1)[row_offsets[r] : row_offsets[r] + length]."""
        h = self.handle(arena.device)
        with torch.cuda.device(arena.device):
            y = out if out is not None else torch.empty(BC, length, dtype=torch.float32, device=arena.device)
            ws = self._scratch("xsq_slicqt_inverse_workspace", arena.device, h, BC, S)
            if out is not None:
                assert row_offsets is not None and row_offsets.dtype == torch.int64 and row_offsets.numel() == BC
                assert out.is_contiguous() and out.dtype == torch.float32
            _lib.call("xsq_slicqt_inverse_rows", h, arena.data_ptr(), BC, S, length, y.data_ptr(),
                      row_offsets.data_ptr() if row_offsets is not None else None, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        return y

    def backward_adjoint(self, gy: Tensor, S: int, out: Tensor = None) -> Tensor:
        """Adjoint of ``backward``: gy (BC, length) = dLoss/dy on a ROCm device -> the arena of dLoss/dcoef for BC channels
        and S slices (xsq_slicqt_inverse_adjoint).  With ``out`` (an arena of that shape) the result is added to it."""
        gy = gy.to(torch.float32).contiguous()
        BC, length = gy.shape
        h = self.handle(gy.device)
        with torch.cuda.device(gy.device):
            if out is not None:
                assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == self.table.numel(BC, S)
            arena = out if out is not None else torch.empty(self.table.numel(BC, S), dtype=torch.float32, device=gy.device)
            ws = self._scratch("xsq_slicqt_inverse_adjoint_workspace", gy.device, h, BC, S, int(out is not None), least=2)
            _lib.call("xsq_slicqt_inverse_adjoint", h, gy.data_ptr(), BC, S, length, arena.data_ptr(), int(out is not None), ws.data_ptr(),
                      ws.numel(), _lib.stream_ptr())
        return arena

    def forward_adjoint(self, garena: Tensor, lead, n: int) -> Tensor:
        """Adjoint of ``forward``: garena = dLoss/dcoef (the real view of the coefficients' cotangent, arena layout for
        prod(lead) channels and num_slices(n) slices) on a ROCm device -> dLoss/dx (*lead, n) fp32 (xsq_slicqt_forward_adjoint)."""
        lead = tuple(lead)
        n = int(n)
        BC = int(np.prod(lead)) if len(lead) else 1
        S = self.plan.num_slices(n)
        h = self.handle(garena.device)
        if garena.dtype != torch.float32 or not garena.is_contiguous() or garena.numel() != self.table.numel(BC, S):
            raise ValueError(f"forward_adjoint: expected a contiguous fp32 arena of {self.table.numel(BC, S)} floats "
                             f"({BC} channels, {S} slices), got {garena.dtype} x {garena.numel()}")
        with torch.cuda.device(garena.device):
            gx = torch.empty(BC, n, dtype=torch.float32, device=garena.device)
            ws = self._scratch("xsq_slicqt_forward_adjoint_workspace", garena.device, h, BC, n)
            _lib.call("xsq_slicqt_forward_adjoint", h, garena.data_ptr(), BC, n, gx.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        return gx.view(*lead, n)

    def backward_masked(self, masks: Tensor, mix: Tensor, BC: int, BCx: int, S: int, length: int, out: Tensor,
                        row_offsets: Tensor) -> Tensor:
        """Inverse transform of masks[bc] * mix[bc % BCx] without materialising the product
        (the separator's mix-phase path): masks = real arena for BC channels, mix = complex arena
        for BCx channels.  Output placement as in ``backward``."""
        h = self.handle(masks.device)
        with torch.cuda.device(masks.device):
            ws = self._scratch("xsq_slicqt_inverse_workspace", masks.device, h, BC, S)
            assert row_offsets.dtype == torch.int64 and row_offsets.numel() == BC
            assert out.is_contiguous() and out.dtype == torch.float32
            _lib.call("xsq_slicqt_inverse_masked", h, masks.data_ptr(), mix.data_ptr(), BC, BCx, S, length, out.data_ptr(),
                      row_offsets.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        return out


class NSGTBase(nn.Module):
    """transforms.py:21-94.  Holds the plan; `.nsgt` is the device engine.  ``dc_twins=True`` accepts a plan with bands across
    DC and computes the reference's mirrored synthesis of them (``plan.build_plan``); the default refuses such a plan.
    ``long_bands=True`` opens the scales ``cqlog`` and ``vqlog`` (``fgamma``: the offset of the latter's centres) and runs the
    bands above 320 on the FFT band engine."""

    def __init__(self, scale, fbins, fmin, fmax=22050.0, fgamma=15.0, fs=44100.0, device="cuda", dc_twins=False, long_bands=False):
        super().__init__()
        self.fbins = fbins
        self.fmin = fmin
        self.fmax = fmax
        self.plan = build_plan(scale, fbins, fmin, fmax, fs, dc_twins=dc_twins, fgamma=fgamma, long_bands=long_bands)
        self.sllen, self.trlen = self.plan.L, self.plan.tr
        print(f"scale={scale}, fbins={fbins}, fmin={fmin:.2f}, fmax={fmax:.2f}, "
              f"sllen={self.sllen}, trlen={self.trlen}")
        self.nsgt = SliCQEngine(self.plan)
        self.M = self.nsgt.ncoefs
        self.fs = fs
        self.fbins_actual = self.nsgt.fbins_actual

    def predict_input_size(self, batch_size, nb_channels, seq_dur_s):
        """transforms.py:80-90.  The block shapes follow from the plan, so no
        transform is run (and the global RNG is left alone);
        the returned list holds zero tensors of the right shapes."""
        n = int(seq_dur_s * self.fs)
        S = self.plan.num_slices(n)
        x = torch.zeros((batch_size, nb_channels, n), dtype=torch.float32)
        jag = [torch.zeros((batch_size, nb_channels, F, S, T, 2), dtype=torch.float32)
               for (_, F, T) in self.plan.blocks]
        return jag, x


def _first_order_only(name):
    """Decorator of a ``Function.backward``: both transforms are linear maps whose adjoints are native calls outside
    autograd, so the backward is once-differentiable; asking for a graph through it raises, naming the transform."""
    def deco(fn):
        once = once_differentiable(fn)

        @functools.wraps(fn)
        def backward(ctx, *grads):
            if torch.is_grad_enabled() and any(g is not None and g.requires_grad for g in grads):
                raise RuntimeError(f"{name}: double backward through the sliCQT is not supported "
                                   f"(the gradient of {name} is a native call without a graph of its own)")
            return once(ctx, *grads)
        return backward
    return deco


class _SliCQForward(torch.autograd.Function):
    """``NSGT_SL.forward`` as one node: the blocks are the zero-copy views of the arena ``SliCQEngine.forward`` fills; the
    backward packs their cotangents into one gradient arena and calls ``SliCQEngine.forward_adjoint``.  The transform is
    linear: nothing but n, lead and S is kept."""

    @staticmethod
    def forward(ctx, eng, x):
        arena, lead, S = eng.forward(x)
        ctx.eng, ctx.lead, ctx.S, ctx.n, ctx.dtype = eng, lead, S, x.shape[-1], x.dtype
        ctx.set_materialize_grads(False)            # a block the loss never touched arrives as None
        return tuple(eng.table.views(arena, lead, S))

    @staticmethod
    @_first_order_only("NSGT_SL")
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return None, None
        dev = next(g for g in grads if g is not None).device
        garena = ctx.eng.table.pack_grads(grads, ctx.lead, ctx.S, dev)
        return None, ctx.eng.forward_adjoint(garena, ctx.lead, ctx.n).to(ctx.dtype)


class _SliCQInverse(torch.autograd.Function):
    """``INSGT_SL.forward`` as one node over all blocks: the packing of ``BlockTable.as_arena`` (zero-copy for a run of views
    of one arena, such as the untouched outputs of ``NSGT_SL``) happens inside the node, and the backward scatters the arena
    of ``SliCQEngine.backward_adjoint`` back to the blocks as views."""

    @staticmethod
    def forward(ctx, eng, length, *blocks):
        arena, lead, S = eng.table.as_arena(list(blocks))
        BC = int(np.prod(lead)) if len(lead) else 1
        ctx.eng, ctx.lead, ctx.S, ctx.BC, ctx.length = eng, lead, S, BC, length
        ctx.dtypes = [b.dtype for b in blocks]
        return eng.backward(arena, BC, S, length).view(*lead, -1)

    @staticmethod
    @_first_order_only("INSGT_SL")
    def backward(ctx, gy):
        if gy is None:
            return (None, None) + (None,) * len(ctx.dtypes)
        garena = ctx.eng.backward_adjoint(gy.reshape(ctx.BC, ctx.length), ctx.S)
        views = ctx.eng.table.views(garena, ctx.lead, ctx.S)
        return (None, None) + tuple(v.to(dt) if need else None
                                    for v, dt, need in zip(views, ctx.dtypes, ctx.needs_input_grad[2:]))


class NSGT_SL(nn.Module):
    """transforms.py:97-131."""

    def __init__(self, nsgt):
        super().__init__()
        self.nsgt = nsgt

    def forward(self, x: Tensor) -> List[Tensor]:
        """(nb_samples, nb_channels, nb_timesteps) -> list over blocks of
        (nb_samples, nb_channels, F_b, nb_slices, T_b, 2), views of one arena.  With grad mode on and ``x`` requiring
        grad the blocks carry the gradient back to ``x`` (one autograd node, same arena, same views)."""
        eng = self.nsgt.nsgt
        if torch.is_grad_enabled() and x.requires_grad:
            return list(_SliCQForward.apply(eng, x))
        arena, lead, S = eng.forward(x)
        return eng.table.views(arena, lead, S)


class INSGT_SL(nn.Module):
    """transforms.py:134-178.  Accepts 6-D (B,C,F,S,T,2) or 7-D (4,B,C,F,S,T,2) blocks."""

    def __init__(self, nsgt):
        super().__init__()
        self.nsgt = nsgt

    def forward(self, X_list, length: int) -> Tensor:
        eng = self.nsgt.nsgt
        X_list = list(X_list)
        if torch.is_grad_enabled() and any(isinstance(X, Tensor) and X.requires_grad for X in X_list):
            return _SliCQInverse.apply(eng, int(length), *X_list)
        arena, lead, S = eng.table.as_arena(X_list)
        BC = int(np.prod(lead)) if len(lead) else 1
        y = eng.backward(arena, BC, S, int(length))
        return y.view(*lead, -1)


class ComplexNorm(nn.Module):
    """transforms.py:181-208: magnitude of a block list or of one tensor."""

    def forward(self, spec):
        if isinstance(spec, list):
            return [torch.abs(torch.view_as_complex(b)) for b in spec]
        if isinstance(spec, Tensor):
            return self.forward([spec])[0]
        raise ValueError(f"unsupported type for 'spec': {type(spec)}")
