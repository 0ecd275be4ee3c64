"""Trained-like CDAE weights for the float64 parity tests (tests/test_stress_weights_cpu.py, tests/test_ref64_stress_gpu.py).

TEST INFRASTRUCTURE (see oracle/__init__.py).  ``xumx_slicq_amd.weights.seeded_state_dict`` is benign on purpose: positive BatchNorm
gammas, running variances five orders of magnitude above eps, one gain for every channel, masks away from 0 and 1.  A trained
checkpoint has dead channels (running variance far below eps), negative and zero gammas, whitening scales over decades and masks
pinned at 0 and 1.  ``stress_state_dict`` draws such weights, ``calibrated`` sets every BatchNorm running statistic to the float64
batch statistic of its layer on a clip, so that the activations stay O(1) (without it the masks saturate into insensitivity) and a
dead channel has running_var = 0 EXACTLY with running_mean = its constant output: the one place where gamma / sqrt(var + eps) is
316 gamma and the folded shift  beta - mean * s  has to cancel.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, Tuple

import numpy as np
import torch

from . import model as omodel
from . import ref64

DEAD_SHARE = 0.10            # conv output channels with gain exactly 0 (dead=True)
NEG_GAMMA, ZERO_GAMMA = 0.35, 0.05


def _logu(rng, a, b, shape):
    return np.exp(rng.uniform(np.log(a), np.log(b), shape))


def stress_state_dict(blocks: Iterable[Tuple[int, int]], seed: int = 4321, dead: bool = True) -> "OrderedDict[str, torch.Tensor]":
    """Every tensor of the state_dict in key order from ONE PCG64(seed) stream (keys, order and shapes of ``state_dict_spec``).

    Layers 1-3: the seeded rule's Kaiming-uniform draw times a gain per OUTPUT channel (axis 0 of a Conv2d, axis 1 of a
    ConvTranspose2d), logU[1e-3, 3] with 10 % of the gains exactly 0 (``dead=True``) or logU[0.1, 3], none zero (``dead=False``, the
    training dict: a zero-gain channel has batch variance 0 and makes the float64 reference itself ill-conditioned).  Layer 4: the
    seeded bound times 3, bias U[-4, 4].  BatchNorm gamma logU[0.05, 4], negative with probability 0.35, zero with 0.05; beta
    U[-1, 1]; running statistics 0 / 1 (to be calibrated) or the seeded rule's (``dead=False``).  input_mean U[-3, 0], input_scale
    logU[0.05, 20]."""
    from xumx_slicq_amd.weights import state_dict_spec
    rng = np.random.default_rng(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for key, shape, kind in state_dict_spec(blocks):
        if kind == "bn_n":
            sd[key] = torch.tensor(100, dtype=torch.long)
            continue
        if kind in ("conv", "convT"):
            ax = 0 if kind == "conv" else 1              # the output channel
            fan_in = shape[1 - ax] * shape[2] * shape[3]
            bound = np.sqrt(6.0 / fan_in)
            a = rng.uniform(-bound, bound, shape)
            gain = _logu(rng, 1e-3 if dead else 0.1, 3.0, shape[ax])
            kill = rng.uniform(0.0, 1.0, shape[ax]) < DEAD_SHARE
            if dead:
                gain[kill] = 0.0
            a = a * gain.reshape([-1 if d == ax else 1 for d in range(4)])
        elif kind == "convT_out":
            bound = 3.0 * np.sqrt(6.0 / (shape[0] * shape[2] * 2))
            a = rng.uniform(-bound, bound, shape)
        elif kind == "out_bias":
            a = rng.uniform(-4.0, 4.0, shape)
        elif kind == "bn_w":
            a = _logu(rng, 0.05, 4.0, shape)
            u = rng.uniform(0.0, 1.0, shape)
            a = np.where(u < NEG_GAMMA, -a, a)
            a = np.where(rng.uniform(0.0, 1.0, shape) < ZERO_GAMMA, 0.0, a)
        elif kind == "bn_b":
            a = rng.uniform(-1.0, 1.0, shape)
        elif kind == "bn_m":
            a = np.zeros(shape) if dead else rng.uniform(-0.2, 0.2, shape)
        elif kind == "bn_v":
            a = np.ones(shape) if dead else rng.uniform(0.5, 1.5, shape)
        elif kind == "in_mean":
            a = rng.uniform(-3.0, 0.0, shape)
        elif kind == "in_scale":
            a = _logu(rng, 0.05, 20.0, shape)
        else:  # pragma: no cover
            raise AssertionError(kind)
        sd[key] = torch.from_numpy(np.asarray(a).astype(np.float32))
    return sd


def calibration_clip() -> torch.Tensor:
    from xumx_slicq_amd.synth import synth_audio
    return synth_audio(30000, seed=777, nb_samples=1)


def calibrated(sd: Dict[str, torch.Tensor], plan, causal: bool, clip: torch.Tensor = None) -> "OrderedDict[str, torch.Tensor]":
    """A copy of ``sd`` whose BatchNorm running_mean / running_var are the float64 batch statistics (biased variance, what the
    layer normalises with in training mode) of each layer on ``clip`` (B, 2, n), rounded to fp32.  Layer 1 differs between the causal
    and the offline model: one calibrated dict per model."""
    clip = calibration_clip() if clip is None else clip
    out = OrderedDict((k, v.clone()) for k, v in sd.items())
    with torch.no_grad():
        for b, Xb in enumerate(ref64.forward(plan, clip)):
            stats = {}
            omodel.cdae_masks(ref64._sd64(sd, b), b, ref64.abs_of_real_complex(Xb), causal, training=True, stats=stats)
            for key, (mean, var, _, _, _) in stats.items():
                out[key + ".running_mean"] = mean.to(torch.float32)
                out[key + ".running_var"] = var.to(torch.float32)
    return out


def zero_gain_channels(sd: Dict[str, torch.Tensor], b: int) -> int:
    """Number of conv output channels of block ``b`` (layers 1-3, four targets) whose weights are all zero."""
    n = 0
    for t in range(4):
        p = f"sliced_umx.{b}.cdaes.{t}."
        n += int((sd[p + "0.weight"].abs().amax((1, 2, 3)) == 0).sum()) + int((sd[p + "3.weight"].abs().amax((1, 2, 3)) == 0).sum())
        n += int((sd[p + "6.weight"].abs().amax((0, 2, 3)) == 0).sum())
    return n


def smallest_running_var(sd: Dict[str, torch.Tensor], b: int) -> float:
    pre = f"sliced_umx.{b}."
    return min(float(v.min()) for k, v in sd.items() if k.startswith(pre) and k.endswith("running_var"))


def first_dead_channel(sd: Dict[str, torch.Tensor]) -> Tuple[int, int, int]:
    """(block, target, channel) of the first zero-gain output channel of a `6.weight` whose layer-3 gamma is not zero."""
    for key, v in sd.items():
        if key.endswith(".6.weight"):
            _, b, _, t, _, _ = key.split(".")
            gamma = sd[f"sliced_umx.{b}.cdaes.{t}.7.weight"]
            dead = ((v.abs().amax((0, 2, 3)) == 0) & (gamma != 0)).nonzero()
            if len(dead):
                return int(b), int(t), int(dead[0])
    raise AssertionError("no zero-gain output channel in any 6.weight")
