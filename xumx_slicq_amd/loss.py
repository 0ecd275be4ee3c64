"""Mirrors of /root/reference/xumx_slicq_v2/loss.py on the HIP library:
``SDRLossCriterion`` (loss.py:5-34), ``ComplexMSELossCriterion`` (loss.py:37-76) and ``MaskSumLossCriterion``
(loss.py:79-96), plus ``validation_step`` = the body of ``training.loop`` with ``train=False`` (training.py:66-103).
The criteria are forward only; ``sdr_loss_and_gradient`` also returns the SDR criterion's gradient with respect to the
estimated waveforms (the training step forms it inside ``xsq_train_step_sdr``).  The SDR term is the SD-SDR of
``auraloss.time.SDSDRLoss()`` as written out in DESIGN.md section 7: auraloss itself is not a dependency."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .arena import BlockTable
from .phase import _tables, _workspace


def _per_block_losses(pred: Sequence[Tensor], target: Sequence[Tensor], masks: Optional[Sequence[Tensor]]):
    """(nblocks, 2) float64 on the device: per block (complex MSE over the 14 combinations, mask-sum MSE)."""
    table = BlockTable([(p.shape[-4], p.shape[-2]) for p in pred])
    P, lead, S = table.as_arena(list(pred))
    Tg, lead_t, S_t = table.as_arena(list(target))
    if lead != lead_t or S != S_t or len(lead) != 3 or lead[0] != 4 or lead[2] != 2:
        raise ValueError(f"expected (4, nb_samples, 2, F, S, T, 2) blocks for both arguments; got {lead} / {lead_t}")
    if P.device.type != "cuda":
        raise _lib.XsqError("the loss kernels run on a ROCm device only; there is no CPU fallback")
    B = lead[1]
    M = None
    if masks is not None:
        total = table.numel(8 * B, S, complex_=False)
        M = torch.cat([m.to(torch.float32).reshape(-1) for m in masks]) if not _is_run(masks, total) else \
            torch.as_strided(masks[0], (total,), (1,))
    F, T = _tables(table)
    with torch.cuda.device(P.device):
        out = torch.empty(len(table), 2, dtype=torch.float64, device=P.device)
        ws = _workspace(P.device, _lib.workspace_bytes("xsq_loss_workspace", len(table), F.ctypes.data, T.ctypes.data, B, S,
                                                       why=f"bad shape: {len(table)} blocks, B={B}, S={S}"))
        _lib.call("xsq_loss_forward", len(table), F.ctypes.data, T.ctypes.data, P.data_ptr(), Tg.data_ptr(),
                  M.data_ptr() if M is not None else None, B, S, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    return out


def _is_run(ts: Sequence[Tensor], total: int) -> bool:
    """Views laid out back to back in ONE allocation of at least ``total`` floats (tensors of their own that merely sit next to
    each other in the allocator's pool are no run: a view cannot span two storages)."""
    ptr = ts[0].data_ptr()
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() != ptr:
            return False
        ptr += t.numel() * 4
    st = ts[0].untyped_storage()
    return st.nbytes() - (ts[0].data_ptr() - st.data_ptr()) >= total * 4


def _sdr(pred: Tensor, target: Tensor, scale: Optional[float]):
    if pred.shape != target.shape or pred.dim() != 4 or pred.shape[0] != 4 or pred.shape[2] != 2:
        raise ValueError(f"expected (4, nb_samples, 2, nb_timesteps) waveforms for both arguments; got {tuple(pred.shape)} / "
                         f"{tuple(target.shape)}")
    if pred.device.type != "cuda" or target.device != pred.device:
        raise _lib.XsqError("the loss kernels run on a ROCm device only; there is no CPU fallback")
    p = pred.detach().to(torch.float32).contiguous()
    t = target.detach().to(torch.float32).contiguous()
    B, n = p.shape[1], p.shape[3]
    with torch.cuda.device(p.device):
        out = torch.empty(1 + 84 * B, dtype=torch.float64, device=p.device)
        ws = _workspace(p.device, _lib.workspace_bytes("xsq_sdr_loss_workspace", B, n, why=f"bad shape B={B} n={n}"))
        if scale is None:
            _lib.call("xsq_sdr_loss_forward", p.data_ptr(), t.data_ptr(), B, n, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
            return out, None
        gy = torch.empty_like(p)
        _lib.call("xsq_sdr_loss_backward", p.data_ptr(), t.data_ptr(), B, n, float(scale), out.data_ptr(), gy.data_ptr(), ws.data_ptr(),
                  ws.numel(), _lib.stream_ptr())
    return out, gy


def sdr_loss_and_gradient(pred_waveforms: Tensor, target_waveforms: Tensor, scale: float = 1.0):
    """(float64 tensor on the device: the criterion, then its (nb_samples, 2, 14) row losses and, in the same layout, the scalars
    A and B of every combination's gradient A t + B (p - t), flattened; scale * d criterion / d pred_waveforms)."""
    return _sdr(pred_waveforms, target_waveforms, scale)


class SDRLossCriterion:
    """loss.py:5-34: mean SD-SDR loss over the 14 one-, two- and three-target sums of (4, nb_samples, 2, nb_timesteps)
    waveforms.  The sums are never formed: two streaming passes over the eight waveforms of a row (csrc/sdr.hip)."""

    def __call__(self, pred_waveforms: Tensor, target_waveforms: Tensor) -> Tensor:
        return _sdr(pred_waveforms, target_waveforms, None)[0][0].float()


class ComplexMSELossCriterion:
    """loss.py:37-76."""

    def __call__(self, pred_complex: List[Tensor], target_complex: List[Tensor]) -> Tensor:
        return _per_block_losses(pred_complex, target_complex, None)[:, 0].mean().float()


class MaskSumLossCriterion:
    """loss.py:79-96."""

    def __call__(self, Ymasks: List[Tensor]) -> Tensor:
        # the mask term only needs the masks; reuse the fused kernel with pred == target == any complex arena
        zeros = [torch.zeros(*m.shape, 2, dtype=torch.float32, device=m.device) for m in Ymasks]
        return _per_block_losses(zeros, zeros, Ymasks)[:, 1].mean().float()


@torch.no_grad()
def validation_step(unmix, encoder, x: Tensor, y_targets: Tensor, sdr_mcoef: float = -1.0):
    """training.py:66-103 with train=False (unmix.eval(), no grad):
    x (B, 2, N) mix, y_targets (4, B, 2, N) -> (loss, mse_loss, mask_loss) as python floats.
    Both criteria come out of one fused streaming pass over the estimate / target / mask arenas.
    ``sdr_mcoef > 0`` (the reference's rule, training.py:94) adds ``sdr_mcoef * SDRLossCriterion()(insgt(estimates), y_targets)``
    and returns (loss, mse_loss, mask_loss, sdr_loss), ``sdr_loss`` unweighted."""
    nsgt, insgt, cnorm = encoder
    Xcomplex = nsgt(x)
    Ycomplex_ests, Ymasks = unmix(Xcomplex, return_masks=True)
    Ycomplex_targets = nsgt(y_targets)
    per_block = _per_block_losses(Ycomplex_ests, Ycomplex_targets, Ymasks)
    mse, mask = (float(v) for v in per_block.mean(dim=0).cpu())
    if not sdr_mcoef > 0:
        return mse + mask, mse, mask
    y_ests = insgt(Ycomplex_ests, x.shape[-1])
    sdr = float(_sdr(y_ests, y_targets.to(y_ests.device), None)[0][0].cpu())
    return mse + mask + float(sdr_mcoef) * sdr, mse, mask, sdr
