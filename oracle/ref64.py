"""Float64 reference of the demix hot path: sliCQT, CDAE masks, post-filters, the whole chain for one chunk.

TEST INFRASTRUCTURE (see oracle/__init__.py).  The fp32 oracle (oracle/slicqt.py, oracle/model.py) is pinned to the
reference, but it rounds like the kernels do, so a comparison against it cannot hold a kernel tighter than a few
thousand fp32 roundings.  This module restates the same closed forms (the docstrings of ``oslicqt.forward`` /
``oslicqt.inverse``, ``omodel.cdae_masks``, ``omodel.norbert_wiener``) in float64 / complex128 on the SAME tables: the
analysis windows ``g`` and the slice window ``tw`` are the plan's fp32 values promoted to float64, the dual windows
``gd`` are fp64 already, the weights are the fp32 state dict promoted.  Against it the error of an fp32 implementation
is its arithmetic alone; ``rel_err`` is the one metric every test of that kind uses.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import model as omodel
from . import slicqt as oslicqt

F64, C128 = torch.float64, torch.complex128


# --------------------------------------------------------------------------
# metric
# --------------------------------------------------------------------------
def rel_err(got: torch.Tensor, ref: torch.Tensor, keep: Sequence[int] = ()) -> Tuple[np.ndarray, np.ndarray]:
    """(rel_rms, rel_max) of ``got`` against ``ref``, one value per index of the dimensions ``keep`` (all others are
    pooled; ``keep=()`` gives two scalars): rel_rms = rms(got - ref) / rms(ref), rel_max = max|got - ref| / rms(ref).
    Everything is promoted to float64 before the first subtraction.  A group whose reference is all zero has no scale:
    that is an error of the test, not a result."""
    g = got.detach().to("cpu", F64)
    r = ref.detach().to("cpu", F64)
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    keep = tuple(k % r.dim() for k in keep)
    pool = tuple(d for d in range(r.dim()) if d not in keep)
    d = g - r
    if not pool:
        raise ValueError("rel_err: nothing to pool over")
    ref_rms = r.pow(2).mean(pool).sqrt()
    if not bool((ref_rms > 0).all()):
        raise ValueError("rel_err: a group of the reference is identically zero")
    return (d.pow(2).mean(pool).sqrt() / ref_rms).numpy(), (d.abs().amax(pool) / ref_rms).numpy()


def band_rel_err(got: List[torch.Tensor], ref: List[torch.Tensor], per_row: bool = False):
    """``rel_err`` per band over a block list of (*lead, F_b, S, T_b, 2) tensors: two arrays of nbands values (pooled
    over the leading dimensions), or of prod(lead) x nbands values with ``per_row``."""
    rms, mx = [], []
    for a, b in zip(got, ref):
        F = b.shape[-4]
        a = a.reshape(-1, F, *b.shape[-3:])
        b = b.reshape(-1, F, *b.shape[-3:])
        r, m = rel_err(a, b, keep=(0, 1) if per_row else (1,))
        rms.append(r)
        mx.append(m)
    return np.concatenate(rms, axis=-1), np.concatenate(mx, axis=-1)


# --------------------------------------------------------------------------
# sliCQT
# --------------------------------------------------------------------------
def forward(plan: oslicqt.Plan, x: torch.Tensor) -> List[torch.Tensor]:
    """x (..., n) -> list over blocks of (..., F_b, S, T_b, 2) float64: the closed form of ``oslicqt.forward``,
      coef[s,ch,j,:] = (-1)^(c_j/2) IFFT_Lg( g_j[q] U_s[(c_j+sq(q)) mod L] ),  U_s = FFT_L( tw * xpad[(2s-2)h : (2s+2)h] )."""
    lead = x.shape[:-1]
    n = x.shape[-1]
    xb = x.reshape(-1, n).to(F64)
    L, h = plan.L, plan.h
    S = plan.nslices(n)
    xpad = torch.zeros(xb.shape[0], (2 * S + 2) * h, dtype=F64)
    xpad[:, 2 * h: 2 * h + n] = xb
    seg = xpad.unfold(-1, L, 2 * h)[:, :S]                                   # (BC, S, L)
    U = torch.fft.fft(seg * torch.from_numpy(plan.tw).to(F64))
    out = []
    for (j0, F, T) in plan.blocks:
        sq = oslicqt._sq(T)
        idx = torch.from_numpy((plan.c[j0:j0 + F, None] + sq[None, :]) % L)
        gw = torch.from_numpy(np.stack(plan.g[j0:j0 + F])).to(F64)
        sign = torch.from_numpy(np.where((plan.c[j0:j0 + F] // 2) % 2 == 0, 1.0, -1.0))
        cb = torch.fft.ifft(U[:, :, idx] * gw) * sign[None, None, :, None]
        cb = cb.permute(0, 2, 1, 3).contiguous()                             # (BC, F, S, T)
        out.append(torch.view_as_real(cb).reshape(*lead, F, S, T, 2))
    return out


def inverse(plan: oslicqt.Plan, X_list: List[torch.Tensor], length: int, twins=None) -> torch.Tensor:
    """list of (*lead, F_b, S, T_b, 2) -> (*lead, length) float64: the closed form of ``oslicqt.inverse``,
      fr_s[c_j+sq(q)] += (-1)^(c_j/2) Lg gd_j[q] FFT_Lg(coef_s,j)[q]  (bins 0..L/2);  seg_s = irfft_L(fr_s);
      y[(2s-2)h + p] += seg_s[p],
    and for the bands that reach across DC (``plan.twins``) the kept part of the reference's mirrored synthesis,
      fr_s[q - c_j] += (-1)^(c_j/2) (-1)^q (-i)^(+-1) Lg gd'_j[q] conj(FFT_Lg(coef_s,j)[q + 1])  (c_j <= q < Lg/2; -i on even
    slices, +i on odd ones).  ``twins`` as in ``oslicqt.inverse``."""
    L, h = plan.L, plan.h
    lead = X_list[0].shape[:-4]
    S = X_list[0].shape[-3]
    BC = int(np.prod(lead)) if len(lead) else 1
    fr = torch.zeros(BC, S, L // 2 + 1, dtype=C128)
    live = plan.live_twins() if twins is None else (plan.twins if twins else [])
    for (j0, F, T), Xb in zip(plan.blocks, X_list):
        cb = torch.view_as_complex(Xb.to(F64).reshape(BC, F, S, T, 2).contiguous())
        fc = torch.fft.fft(cb)
        sq = oslicqt._sq(T)
        for f in range(F):
            j = j0 + f
            sign = 1.0 if (plan.c[j] // 2) % 2 == 0 else -1.0
            w = torch.from_numpy(plan.gd[j] * (T * sign)).to(C128)
            k = plan.c[j] + sq
            keep = (k >= 0) & (k <= L // 2)
            fr[:, :, torch.from_numpy(k[keep])] += (fc[:, f] * w)[:, :, torch.from_numpy(keep)]
        for (j, q, k, gdm) in live:
            if j0 <= j < j0 + F:
                sign = 1.0 if (plan.c[j] // 2) % 2 == 0 else -1.0
                w = torch.from_numpy(gdm * (T * sign) * np.where(q % 2 == 0, 1.0, -1.0)).to(C128)
                rot = torch.tensor([-1j if s % 2 == 0 else 1j for s in range(S)], dtype=C128)
                fr[:, :, torch.from_numpy(k)] += fc[:, j - j0][:, :, torch.from_numpy(q + 1)].conj() * w * rot[None, :, None]
    seg = torch.fft.irfft(fr, n=L)
    y = torch.zeros(BC, (2 * S + 2) * h, dtype=F64)
    for s in range(S):
        y[:, 2 * s * h: 2 * s * h + L] += seg[:, s]
    return y[:, 2 * h: 2 * h + length].reshape(*lead, length)


# --------------------------------------------------------------------------
# CDAE
# --------------------------------------------------------------------------
_SD64 = {}


def _sd64(sd: Dict[str, torch.Tensor], b: int) -> Dict[str, torch.Tensor]:
    """The tensors of block ``b`` promoted to float64, cached per (state dict, block)."""
    key = (id(sd), b)
    hit = _SD64.get(key)
    if hit is None or hit[0] is not sd:
        pre = f"sliced_umx.{b}."
        hit = _SD64[key] = (sd, {k: v.to(F64) for k, v in sd.items() if k.startswith(pre) and v.is_floating_point()})
    return hit[1]


def cdae_masks(sd: Dict[str, torch.Tensor], b: int, mag: torch.Tensor, causal: bool) -> torch.Tensor:
    """mag (B, 2, F, S, T) -> sigmoid masks (4, B, 2, F, S, T) float64: ``omodel.cdae_masks`` itself, run on the
    promoted state dict (every op in it follows the dtype of its operands)."""
    with torch.no_grad():
        return omodel.cdae_masks(_sd64(sd, b), b, mag.to(F64), causal)


def cdae_logits(masks: torch.Tensor) -> torch.Tensor:
    """The layer-4 pre-activation of float64-promoted masks, log(m / (1 - m)); for diagnosis of a failed mask comparison
    only: meaningful where the mask is away from 0 and 1 (the tests look at (0.02, 0.98))."""
    m = masks.to(F64)
    return torch.log(m) - torch.log1p(-m)


# --------------------------------------------------------------------------
# post-filters
# --------------------------------------------------------------------------
def phasemix_sep(X: torch.Tensor, Ymag: torch.Tensor) -> torch.Tensor:
    """X (B,2,F,S,T,2), Ymag (4,B,2,F,S,T) -> Ymag * exp(i angle(X)) as (4,B,2,F,S,T,2) float64."""
    return omodel.phasemix_sep(X.to(F64), Ymag.to(F64))


def blockwise_wiener(X: torch.Tensor, Ymag: torch.Tensor, win_len: int = omodel.WIENER_WIN) -> torch.Tensor:
    """``omodel.blockwise_wiener`` in complex128, quirks kept: the regulariser is eps of FLOAT32 (and its square root),
    the window maximum is shared over the batch, and the scale is max(1, 0.1 max|x|) per window (``omodel.norbert_wiener``
    and ``omodel._em_one_iteration`` follow the dtype of their operands and are used as they are)."""
    B, C, Fb, S, T, _ = X.shape
    x = torch.view_as_complex(X.to(F64).reshape(B, C, Fb, S * T, 2).contiguous()).permute(0, 3, 2, 1)   # (B,N,F,C)
    v = Ymag.to(F64).reshape(4, B, C, Fb, S * T).permute(1, 4, 3, 2, 0)                                  # (B,N,F,C,J)
    N = S * T
    wl = win_len if win_len else N
    y = torch.zeros(B, N, Fb, C, 4, dtype=C128)
    for p in range(0, N, wl):
        y[:, p:p + wl] = omodel.norbert_wiener(v[:, p:p + wl], x[:, p:p + wl])
    return torch.view_as_real(y).permute(4, 0, 3, 2, 1, 5).contiguous().reshape(4, B, C, Fb, S, T, 2)


def abs_of_real_complex(X: torch.Tensor) -> torch.Tensor:
    return omodel.abs_of_real_complex(X.to(F64))


def unmix(sd: Dict[str, torch.Tensor], X_list: List[torch.Tensor], causal: bool, wiener: bool):
    """``omodel.unmix`` in float64: (estimates, masks), lists over blocks."""
    Ys, masks = [], []
    for b, X in enumerate(X_list):
        mag = abs_of_real_complex(X)
        m = cdae_masks(sd, b, mag, causal)
        Ymag = m * mag
        Ys.append(blockwise_wiener(X, Ymag) if wiener else phasemix_sep(X, Ymag))
        masks.append(m)
    return Ys, masks


def separate(plan: oslicqt.Plan, sd: Dict[str, torch.Tensor], audio: torch.Tensor, causal: bool, wiener: bool) -> torch.Tensor:
    """audio (B, 2, n), ONE chunk -> (4, B, 2, n) float64: zero-pad to L/2 + 1 samples, sliCQT, CDAE masks, post-filter,
    inverse sliCQT (``oracle.separator.separate`` with chunk_size >= n)."""
    n = audio.shape[-1]
    a = audio.to(F64)
    min_samples = plan.L // 2 + 1
    if n < min_samples:
        a = torch.cat([a, torch.zeros(*a.shape[:-1], min_samples - n, dtype=F64)], dim=-1)
    with torch.no_grad():
        Y, _ = unmix(sd, forward(plan, a), causal, wiener)
        return inverse(plan, Y, n)


# --------------------------------------------------------------------------
# training step: loss, gradients, BatchNorm statistics, AdamW
# --------------------------------------------------------------------------
def block_gradients(sd: Dict[str, torch.Tensor], b: int, Xb: torch.Tensor, Ytb: torch.Tensor, causal: bool, wiener: bool,
                    nblocks: int, dtype: torch.dtype = F64, params: Dict[str, torch.Tensor] = None):
    """Block ``b``'s share of one training step (``oracle.loss.training_gradients``), from COEFFICIENTS: Xb (B, 2, F, S, T, 2) mix,
    Ytb (4, B, 2, F, S, T, 2) targets.  Both losses are means over blocks, so the share of a block is its own term over
    ``nblocks`` and its gradients do not depend on the other blocks.  Autograd in ``dtype`` over ``omodel.cdae_masks(training=True)``,
    the post-filter and ``oloss.complex_mse`` / ``oloss.mask_sum``; float32 gives the fp32 oracle's arithmetic on the same input.
    Returns (mse_b, mask_b, {key: grad}, {bn key: min |BatchNorm output|}, {bn key: (batch mean, biased batch variance, count,
    running_mean, running_var after the step as F.batch_norm(training=True) leaves them)}).  ``params`` (the block's tensors in
    ``dtype``) replaces the promoted state dict: the finite-difference test moves them."""
    from . import loss as oloss
    pre = f"sliced_umx.{b}."
    if params is None:
        params = {k: v.to(dtype) for k, v in sd.items() if k.startswith(pre) and v.is_floating_point()}
    p = {k: (v.detach().clone().requires_grad_(True) if k.endswith(oloss.TRAINABLE_SUFFIXES) else v) for k, v in params.items()}
    minima, stats = {}, {}
    X = Xb.to(dtype)
    mag = omodel.abs_of_real_complex(X)
    m = omodel.cdae_masks(p, b, mag, causal, training=True, minima=minima, stats=stats)
    Ymag = m * mag
    if not wiener:
        Y = omodel.phasemix_sep(X, Ymag)
    elif dtype == F64:
        Y = blockwise_wiener(X, Ymag)
    else:
        Y = omodel.blockwise_wiener(X, Ymag)
    mse = oloss.complex_mse([Y], [Ytb.to(dtype)]) / nblocks
    msk = oloss.mask_sum([m]) / nblocks
    (mse + msk).backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad}
    return float(mse.detach()), float(msk.detach()), grads, minima, stats


def training_gradients(plan: oslicqt.Plan, sd: Dict[str, torch.Tensor], X_list: List[torch.Tensor], Yt_list: List[torch.Tensor],
                       causal: bool, wiener: bool, dtype: torch.dtype = F64):
    """One forward + backward of the training step from the coefficients of the mix and of the targets (lists over blocks):
    (mse, mask, {key: grad}, {bn key: min |BatchNorm output|}, {bn key: statistics}) over all blocks, the loss terms summed in
    float64.  Any of the four (causal, wiener) combinations."""
    nb = len(plan.blocks)
    assert len(X_list) == len(Yt_list) == nb
    mse = msk = 0.0
    grads, minima, stats = {}, {}, {}
    for b in range(nb):
        a, c, g, mi, st = block_gradients(sd, b, X_list[b], Yt_list[b], causal, wiener, nb, dtype)
        mse, msk = mse + a, msk + c
        grads.update(g), minima.update(mi), stats.update(st)
    return mse, msk, grads, minima, stats


def adamw_step(p, g, m, v, step: int, lr: float, wd: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """One ``torch.optim.AdamW`` update in float64 (decoupled decay, bias-corrected moments; the constants are Python doubles):
    returns (p, m, v) after step number ``step`` (1-based)."""
    b1, b2 = betas
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    p = p * (1.0 - lr * wd)
    m = torch.lerp(m, g, 1.0 - b1)
    v = (v * b2).addcmul(g, g, value=1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add(eps)
    return p.addcdiv(m, denom, value=-(lr / bc1)), m, v


def bn_running(old_mean, old_var, batch_mean, batch_var_biased, count: int, momentum: float = 0.1):
    """The running buffers of ``nn.BatchNorm2d.train()`` after one batch, float64: the UNBIASED batch variance goes in."""
    om, ov, bm, bv = (t.to(F64) for t in (old_mean, old_var, batch_mean, batch_var_biased))
    unbiased = bv * (count / (count - 1.0)) if count > 1 else bv
    return (1.0 - momentum) * om + momentum * bm, (1.0 - momentum) * ov + momentum * unbiased


# --------------------------------------------------------------------------
# loss terms per block, dataset statistics per bin
# --------------------------------------------------------------------------
def block_losses(pred: Sequence[torch.Tensor], target: Sequence[torch.Tensor], masks=None, dtype: torch.dtype = F64) -> np.ndarray:
    """Lists over blocks of (4, B, 2, F_b, S, T_b, 2) estimates and targets, and of (4, B, 2, F_b, S, T_b) masks (or None: the
    second column is 0) -> (nblocks, 2) float64: per block ``oracle.loss.complex_mse`` and ``oracle.loss.mask_sum`` of that block
    alone, which is the term the two criteria average over the blocks.  The two functions follow the dtype of their operands:
    float32 is the fp32 oracle's arithmetic, float64 the reference."""
    from . import loss as oloss
    out = np.zeros((len(pred), 2), dtype=np.float64)
    for b, (p, t) in enumerate(zip(pred, target)):
        out[b, 0] = float(oloss.complex_mse([p.to(dtype)], [t.to(dtype)]))
        if masks is not None:
            out[b, 1] = float(oloss.mask_sum([masks[b].to(dtype)]))
    return out


def magnitude_sums(X_list: Sequence[torch.Tensor], dtype: torch.dtype = F64) -> List[np.ndarray]:
    """List over blocks of (C, F_b, S, T_b, 2) coefficients of ONE track (leading dimensions of one are dropped) -> per block
    (F_b, 2) float64: sum and sum of squares over the S * T_b frames of the channel-mean magnitude, what
    ``oracle.statistics.get_statistics`` accumulates per track.  float32: magnitude (``oslicqt.complex_norm``) and channel mean in
    fp32, the sums in float64, as the oracle has them; float64: all of it in float64."""
    out = []
    for X in X_list:
        C, Fb, S, T, _ = X.shape[-5:]
        mag = oslicqt.complex_norm(X.to(dtype).reshape(C, Fb, S * T, 2).contiguous())
        m = mag.mean(0).to(F64)
        out.append(torch.stack((m.sum(1), (m * m).sum(1)), dim=1).numpy())
    return out


def statistics_from_sums(sums: Sequence[np.ndarray], frames: Sequence[float]):
    """The host formula of ``oracle.statistics.get_statistics`` on per-block (F_b, 2) sums merged over the tracks and the frame
    count of each block: (means, stds), population std floored at 1e-4 of the block's largest."""
    means = [s[:, 0] / n for s, n in zip(sums, frames)]
    stds = [np.sqrt(np.maximum(s[:, 1] / n - mu * mu, 0.0)) for s, n, mu in zip(sums, frames, means)]
    return means, [np.maximum(s, 1e-4 * np.max(s)) for s in stds]
