"""Drop-in mirror of /root/reference/xumx_slicq_v2/phase.py on the HIP library:
blockwise_wiener, blockwise_phasemix_sep, abs_of_real_complex (+ the list
helpers wiener / phasemix_sep).  ROCm tensors only; inputs are never modified
(the reference's _atan2 writes into its X argument).
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .arena import BlockTable

SCRATCH = _lib.Scratch()      # the workspaces of this module's calls and of loss.py, statistics.py and slicqfinder.py


def _workspace(device, nbytes):
    return SCRATCH.get(device, nbytes)


def _tables(table: BlockTable):
    F = np.asarray([s[0] for s in table.shapes], dtype=np.int32)
    T = np.asarray([s[1] for s in table.shapes], dtype=np.int32)
    return F, T


def _need_gpu(t: Tensor, who: str):
    if t.device.type != "cuda":
        raise _lib.XsqError(f"{who} runs on a ROCm device only (got '{t.device}'); there is no CPU fallback")


METHODS = {"auto": 0, "looped": 1, "resident": 2}      # the forms of more than one EM iteration (xsq_wiener_em_iter)


def _niter_method(niter, method):
    niter = int(niter)
    if niter < 0:
        raise _lib.XsqError(f"niter must be >= 0 (got {niter})")
    if method not in METHODS:
        raise ValueError(f"method {method!r} not in {sorted(METHODS)}")
    return niter, METHODS[method]


SOFTMASK, RESIDUAL = 1, 2                              # XSQ_WIENER_SOFTMASK, XSQ_WIENER_RESIDUAL (include/xumx_slicq_hip.h)


def option_flags(softmask=False, residual=False) -> int:
    """The flag word of the post-filter options: ``softmask`` (ratio-mask start, norbert.wiener use_softmask) and ``residual``
    (a fifth source holding what the four targets do not explain, norbert.contrib.residual_model)."""
    return (SOFTMASK if softmask else 0) | (RESIDUAL if residual else 0)


def nb_sources(residual=False) -> int:
    """Sources of the estimates' arena: the four targets, and the residual last when it is on."""
    return 5 if residual else 4


def resident_max_window(nb_sources: int = 4) -> int:
    """Longest window (frames) the window-resident EM kernel holds on chip for ``nb_sources`` sources (4, or 5 with the
    residual: fewer frames per thread fit)."""
    if int(nb_sources) == 4:
        return int(_lib.lib.xsq_wiener_resident_max_window())
    n = int(_lib.lib.xsq_wiener_resident_max_window_sources(int(nb_sources)))
    if n <= 0:
        raise ValueError(f"nb_sources must be 4 or 5 (got {nb_sources})")
    return n


def _em(table: BlockTable, X: Tensor, masks, Y: Tensor, B: int, S: int, win_len: int, batch_group: int, niter: int, meth: int, flags: int = 0):
    """Workspace query, workspace and call of the entry point that (``masks is None``, ``niter``) select: one iteration is
    xsq_wiener_em / xsq_wiener_em_masked, any other count the ``_iter`` form of the same; an option set (``flags``) the
    ``_options`` form."""
    F, T = _tables(table)
    geometry = (len(table), F.ctypes.data, T.ctypes.data)
    name, arenas = "xsq_wiener_em", (X.data_ptr(), Y.data_ptr())
    if masks is not None:
        name, arenas = "xsq_wiener_em_masked", (X.data_ptr(), masks.data_ptr(), Y.data_ptr())
    query, count = "xsq_wiener_workspace", ()
    if flags:
        name, query, count = name + "_options", "xsq_wiener_options_workspace", (niter, meth, flags)
    elif niter != 1:
        name, query, count = name + "_iter", "xsq_wiener_iter_workspace", (niter, meth)
    ext_max = (None,) if count and masks is not None else ()          # the masked _iter / _options forms take a table; none here
    with torch.cuda.device(X.device):
        ws = _workspace(X.device, _lib.workspace_bytes(query, *geometry, B, S, win_len, *count, why="bad arguments"))
        _lib.call(name, *geometry, *arenas, B, S, win_len, int(batch_group), *ext_max, *count, ws.data_ptr(), ws.numel(), _lib.stream_ptr())


def wiener_em_arena(table: BlockTable, X: Tensor, Y: Tensor, B: int, S: int, win_len: int = 5000,
                    batch_group: int = 0, niter: int = 1, method: str = "auto", softmask: bool = False, residual: bool = False):
    """``niter`` EM iterations in place on the estimates arena Y (8B channels) given the
    mix arena X (2B channels).  phase.py:43-59 + norbert/__init__.py:153-260 (the reference calls it with one).
    ``batch_group``: runs of that many batch items share the window maximum (0 = whole batch).
    ``niter`` = 0 leaves Y alone, 1 is the reference's call; ``method`` ("auto", "looped", "resident") picks the form of
    ``niter`` >= 2 (include/xumx_slicq_hip.h, xsq_wiener_em_iter).  ``residual``: Y has 10B channels, the residual's start
    last (``wiener_start_arena`` writes the starts of an option set); ``softmask`` belongs to the start and changes nothing here."""
    niter, meth = _niter_method(niter, method)
    if niter:
        _em(table, X, None, Y, B, S, win_len, batch_group, niter, meth, option_flags(False, residual))


def wiener_start_arena(table: BlockTable, X: Tensor, mag: Tensor, Y: Tensor, B: int, S: int, softmask: bool = False, residual: bool = False):
    """The initial estimates of an option set from the magnitudes ``mag`` (real arena, 8B channels) into Y (8B channels, 10B
    with ``residual``): norbert.wiener :247-251 after contrib.residual_model.  At least one option (``xsq_phasemix`` is the
    start without)."""
    F, T = _tables(table)
    with torch.cuda.device(X.device):
        _lib.call("xsq_wiener_start", len(table), F.ctypes.data, T.ctypes.data, X.data_ptr(), mag.data_ptr(), Y.data_ptr(), B, S,
                  option_flags(softmask, residual), _lib.stream_ptr())


def wiener_em_masked_arena(table: BlockTable, X: Tensor, masks: Tensor, Y: Tensor, B: int, S: int, win_len: int = 5000,
                           batch_group: int = 0, niter: int = 1, method: str = "auto", softmask: bool = False, residual: bool = False):
    """The same iteration fed by the sigmoid masks (real arena, 8B channels): the initial estimate mask * X
    (model.py:262-264) is formed while the two passes load, Y (8B channels, complex) is only written.
    Same bits as ``xsq_cdae_forward(Y)`` + ``wiener_em_arena``; a third less HBM traffic.  ``niter`` >= 1, ``method``:
    as ``wiener_em_arena``.  ``softmask`` / ``residual``: the option set, formed from the masks as the frames are loaded
    (v_j = m_j |x|); Y then has 10B channels with ``residual``, and ``niter`` = 0 writes the starts."""
    niter, meth = _niter_method(niter, method)
    _em(table, X, masks, Y, B, S, win_len, batch_group, niter, meth, option_flags(softmask, residual))


def _one_block(mix_slicqt: Tensor, slicqtgrams: Tensor):
    if mix_slicqt.dim() != 6 or mix_slicqt.shape[-1] != 2 or mix_slicqt.shape[1] != 2:
        raise ValueError(f"mix must be (nb_samples, 2, F, S, T, 2); got {tuple(mix_slicqt.shape)}")
    B, _, F, S, T, _ = mix_slicqt.shape
    if tuple(slicqtgrams.shape) != (4, B, 2, F, S, T):
        raise ValueError(f"magnitudes must be (4, {B}, 2, {F}, {S}, {T}); got {tuple(slicqtgrams.shape)}")
    _need_gpu(mix_slicqt, "phase")
    return BlockTable([(F, T)]), B, S


def blockwise_phasemix_sep(X_block: Tensor, Ymag_block: Tensor) -> Tensor:
    """phase.py:96-113: Y = Ymag * exp(i angle(X)).  (B,2,F,S,T,2), (4,B,2,F,S,T) -> (4,B,2,F,S,T,2)."""
    table, B, S = _one_block(X_block, Ymag_block)
    F, T = _tables(table)
    X = X_block.contiguous().float()
    mag = Ymag_block.contiguous().float()
    with torch.cuda.device(X.device):
        Y = torch.empty(*Ymag_block.shape, 2, dtype=torch.float32, device=X.device)
        _lib.call("xsq_phasemix", 1, F.ctypes.data, T.ctypes.data, X.data_ptr(), mag.data_ptr(), Y.data_ptr(), B, S, _lib.stream_ptr())
    return Y


def blockwise_wiener(mix_slicqt: Tensor, slicqtgrams: Tensor, wiener_win_len_param: int = 5000, niter: int = 1,
                     method: str = "auto", softmask: bool = False, residual: bool = False) -> Tensor:
    """phase.py:18-69.  (B,2,F,S,T,2), (4,B,2,F,S,T) -> (4,B,2,F,S,T,2).  ``niter`` (extension; the reference pins 1): the
    iteration count of norbert.wiener, 0 = the initial estimate; ``method``: "auto", "looped" or "resident" for
    ``niter`` >= 2 (``wiener_em_arena``).  ``softmask`` (extension): norbert.wiener's use_softmask; ``residual`` (extension):
    the magnitudes first go through norbert.contrib.residual_model(v, x, 1) and the result is (5,B,2,F,S,T,2), residual last."""
    table, B, S = _one_block(mix_slicqt, slicqtgrams)
    X = mix_slicqt.contiguous().float()
    nb_frames = S * mix_slicqt.shape[4]
    win = int(wiener_win_len_param) if wiener_win_len_param else nb_frames
    if softmask or residual:
        mag = slicqtgrams.contiguous().float()
        with torch.cuda.device(X.device):
            Y = torch.empty(nb_sources(residual), *mag.shape[1:], 2, dtype=torch.float32, device=X.device)
        wiener_start_arena(table, X.view(-1), mag.view(-1), Y.view(-1), B, S, softmask=softmask, residual=residual)
    else:
        Y = blockwise_phasemix_sep(X, slicqtgrams)
    wiener_em_arena(table, X.view(-1), Y.view(-1), B, S, win, niter=niter, method=method, residual=residual)
    return Y


def abs_of_real_complex(Xcomplex_real_view: Tensor) -> Tensor:
    """phase.py:116-118."""
    return torch.sqrt(Xcomplex_real_view[..., 0] ** 2 + Xcomplex_real_view[..., 1] ** 2)


def wiener(mix_slicqt: List[Tensor], slicqtgrams: List[Tensor], wiener_win_len: int = 5000, niter: int = 1, method: str = "auto",
           softmask: bool = False, residual: bool = False):
    """phase.py:7-15."""
    return [blockwise_wiener(m, s, wiener_win_len, niter, method, softmask, residual) for m, s in zip(mix_slicqt, slicqtgrams)]


def phasemix_sep(X: List[Tensor], Ymag: List[Tensor]):
    """phase.py:121-126."""
    return [blockwise_phasemix_sep(x, y) for x, y in zip(X, Ymag)]
