"""Host side of the front end's resampler (xumx_slicq_amd/resample.py, torchaudio.transforms.Resample of data.py:148-156):
the compacted filter table against a float64 restatement of torchaudio's full polyphase table, the geometry (width, span,
output length), the size limit, and the nn.Module's argument rules.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from xumx_slicq_amd import resample as R

MODEL = 44100
PAIRS = [(r, MODEL) for r in (8000, 22050, 32000, 48000, 88200, 96000, 192000)] + [(MODEL, 48000), (MODEL, 22050)]
# width and the longest non-zero run of fp32 taps per phase, input rate -> 44.1 kHz
GEOMETRY = {8000: (7, 13), 22050: (7, 13), 32000: (7, 13), 48000: (7, 14), 88200: (13, 25), 96000: (14, 27),
            192000: (27, 53)}


# ---- float64 restatement of torchaudio's sinc / Hann kernel (lowpass_filter_width 6, rolloff 0.99) --------------------
def ref_geometry(orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    return o, n, base, math.ceil(6 * o / base)


def ref_full_table(orig, new):
    """K[p, k], n x (2*width + o), float32: every tap torchaudio's conv1d multiplies."""
    o, n, base, width = ref_geometry(orig, new)
    idx = np.arange(-width, width + o, dtype=np.float64) / o
    ph = np.arange(0, -n, -1, dtype=np.int64).astype(np.float32) / np.float32(n)     # (a): int / int -> float32
    t = ph.astype(np.float64)[:, None] + idx[None, :]
    t = np.clip(t * base, -6.0, 6.0)
    w = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(t == 0, 1.0, np.sin(t) / t)
    return (s * (w * (base / o))).astype(np.float32)


def ref_length(orig, new, L):
    o, n, _, _ = ref_geometry(orig, new)
    return int(np.ceil(np.float32(n * L / o)))                                           # (b): float32 before the ceiling


def expand(tab):
    full = np.zeros((tab.new, 2 * tab.width + tab.orig), dtype=np.float32)
    for p in range(tab.new):
        f = int(tab.first_tap[p])
        keep = min(tab.span, full.shape[1] - f)
        full[p, f:f + keep] = tab.table[p, :keep]
        assert not tab.table[p, keep:].any()                                             # past the full table: zeros
    return full


@pytest.mark.parametrize("orig,new", PAIRS)
def test_compact_table_expands_to_the_full_table(orig, new):
    tab = R.resample_table(orig, new)
    o, n, _, width = ref_geometry(orig, new)
    full = ref_full_table(orig, new)
    assert (tab.orig, tab.new, tab.width) == (o, n, width)
    assert tab.table.dtype == np.float32 and tab.table.shape == (n, tab.span) and tab.first_tap.dtype == np.int32
    assert np.array_equal(expand(tab), full)
    nz = full != 0
    first = nz.argmax(1)
    last = full.shape[1] - 1 - nz[:, ::-1].argmax(1)
    assert nz.any(1).all() and np.array_equal(first, tab.first_tap)
    assert tab.span == int((last - first).max()) + 1
    for p in range(n):                                                  # outside the kept range: exactly 0
        f = tab.first_tap[p]
        assert not full[p, :f].any() and not full[p, f + tab.span:].any()


@pytest.mark.parametrize("rate", sorted(GEOMETRY))
def test_geometry_and_output_length(rate):
    tab = R.resample_table(rate, MODEL)
    assert (tab.width, tab.span) == GEOMETRY[rate]
    o = tab.orig
    for L in (0, 1, 5, tab.width - 1, o - 1, o, 30011, 10 * rate, 240 * rate, 11_520_007):
        assert tab.output_length(L) == ref_length(rate, MODEL, L), (rate, L)
    if rate == 48000:
        assert tab.output_length(240 * 48000) == 10_584_000
        assert tab.output_length(11_520_007) == 10_584_006          # the exact ceiling would be 10,584,007


def test_near_equal_rates_build_a_compact_table_only():
    """44100 -> 44099: the full table would hold 44099 x 44,114 taps (1.9 G entries); the compact one 44099 x 13."""
    tab = R.resample_table(44100, 44099)
    assert (tab.orig, tab.new) == (44100, 44099)
    assert tab.table.shape == (44099, tab.span) and tab.span <= 16
    assert tab.table.nbytes < 4 << 20
    # spot-check phases against the restatement's taps at those indices
    for p in (0, 1, 22049, 44098):
        k = tab.first_tap[p] + np.arange(tab.span)
        want = R.filter_taps(np.full(tab.span, p), k, tab.orig, tab.new)
        assert np.array_equal(tab.table[p], want)
        assert R.filter_taps(p, tab.first_tap[p] - 1, tab.orig, tab.new) == 0
    with pytest.raises(ValueError, match="entries"):
        R.resample_table(10_000_019, 10_000_079)                   # co-prime rates: 10^7 phases


def test_resample_module_argument_rules():
    x = torch.zeros(2, 100)
    assert R.Resample(44100, 44100)(x) is x
    assert R.Resample(48000.0, torch.as_tensor(48000.0), resampling_method="sinc_interpolation")(x) is x
    assert R.resample(x, 22050, 22050) is x
    for method in ("kaiser_window", "sinc_interp_kaiser", "linear"):
        with pytest.raises(ValueError):
            R.Resample(48000, 44100, resampling_method=method)
    for bad in (44100.5, 0, -8000, float("nan")):
        with pytest.raises(ValueError):
            R.Resample(bad, 44100)
        with pytest.raises(ValueError):
            R.Resample(44100, bad)
    assert R.Resample(48000, 44100, resampling_method="sinc_interp_hann").new_freq == 44100


def test_no_cpu_path():
    """The product has no CPU resampler: a CPU tensor at a foreign rate is refused, with the way out in the message."""
    from xumx_slicq_amd import audio as A
    with pytest.raises(ValueError, match="GPU"):
        R.resample(torch.zeros(2, 100), 48000, 44100)
    with pytest.raises(ValueError, match="device"):
        A.preprocess_audio(torch.zeros(2, 100), rate=48000, model_rate=44100.0)


def test_resample_entry_point_is_declared_and_exported():
    from xumx_slicq_amd import _lib
    assert hasattr(_lib.lib, "xsq_resample") and "xsq_resample" in _lib.EXPORTED
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    assert "int xsq_resample(" in hdr
    # argument checks run on the host: no device memory is touched
    assert _lib.lib.xsq_resample(None, 0, 1, 10, None, 0, 10, None, None, 160, 147, 14, 7, None) < 0
    assert "null" in _lib.last_error()
