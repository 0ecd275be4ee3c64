"""Counterpart of ``separate_sources`` of the reference's Cadenza caller (cadenza/enhance.py:35-99): a
model applied segment by segment, the segments overlapped, faded linearly and added together -- the Demucs / torchaudio
way of joining chunks.  With this package's ``Separator`` at its own sample rate the whole track is ONE native call
(``Separator.forward_overlapped``); any other model takes the loop over ``model.forward``.  The segment rule and its two
departures from the reference text are in DESIGN.md 4.9."""
from __future__ import annotations

import numpy as np
import torch

from .separator import Separator, overlapped_loop, segment_lengths


def separate_sources(model, mix, sample_rate, segment: float = 10.0, overlap: float = 0.1, device=None) -> np.ndarray:
    """enhance.py:35-99.  ``mix``: (batch, channels, time) tensor or array; a 1-D or 2-D ``mix`` gains a batch dimension
    (enhance.py:66-71).  ``device``: where the computation runs (default ``mix.device``, the CPU for an array).
    Returns a numpy array (batch, 4, channels, length)."""
    if device is None:
        device = mix.device if isinstance(mix, torch.Tensor) else torch.device("cpu")
    mix = torch.as_tensor(mix, device=torch.device(device))
    if mix.ndim == 1:                        # one track, mono
        mix = mix[None, None]
    elif mix.ndim == 2:                      # one track
        mix = mix.unsqueeze(0)
    if mix.ndim != 3:
        raise ValueError(f"mix must be (batch, channels, time), (channels, time) or (time,); got {tuple(mix.shape)}")
    if isinstance(model, Separator) and float(sample_rate) == float(model.sample_rate):
        est = model.forward_overlapped(mix, segment, overlap)
    else:
        chunk_len, ov = segment_lengths(sample_rate, segment, overlap)
        with torch.no_grad():
            est = overlapped_loop(model.forward, mix, chunk_len, ov)
    return est.permute(1, 0, 2, 3).cpu().detach().numpy()
