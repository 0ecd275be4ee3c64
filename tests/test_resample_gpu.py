"""The front end's resampler on the MI355X (csrc/resample.hip via xumx_slicq_amd/resample.py): parity with a float64
restatement of torchaudio's sinc / Hann polyphase conv (data.py:148-156), filter properties, a full 240 s track,
preprocess_audio / separate at 48 kHz, and the CLI on a directory of mixed rates."""
import struct
import warnings

import numpy as np
import pytest
import torch

from test_resample_cpu import MODEL, ref_full_table, ref_geometry, ref_length

pytestmark = pytest.mark.gpu

RATES = [(r, MODEL) for r in (8000, 22050, 32000, 48000, 88200, 96000, 192000)] + [(MODEL, 48000)]


def ref_resample(x, orig, new, frames=None):
    """(rows, L) -> (rows, L') in float64: conv1d(x_pad, K, stride o) with x_pad = [width zeros] x [width + o zeros].
    `frames`: only these output frames (j), returned as (rows, len(frames), n)."""
    o, n, _, width = ref_geometry(orig, new)
    K = ref_full_table(orig, new).astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[-1]
    xp = np.concatenate([np.zeros((x.shape[0], width)), x, np.zeros((x.shape[0], width + o))], axis=1)
    win = np.lib.stride_tricks.sliding_window_view(xp, K.shape[1], axis=1)[:, ::o]       # (rows, L // o + 1, taps)
    if frames is not None:
        return np.matmul(win[:, frames], K.T)
    y = np.matmul(win, K.T).reshape(x.shape[0], -1)
    return y[:, :ref_length(orig, new, L)]


def signal(rows, L, seed):
    """Unit-amplitude test input: half the rows uniform noise in [-1, 1], half a synth-like chord with clicks."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (rows, L))
    t = np.arange(L)
    for r in range(1, rows, 2):
        f = rng.uniform(50, 5000, 3) / 48000
        s = sum(np.sin(2 * np.pi * fi * t + rng.uniform(0, 6)) for fi in f) / 3
        s[rng.integers(0, L, max(1, L // 1000))] = 1.0
        x[r] = np.clip(s, -1, 1)
    return x.astype(np.float32)


def run(x, orig, new):
    from xumx_slicq_amd.resample import resample
    y = resample(x, orig, new)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("orig,new", RATES)
def test_parity_with_the_restatement(orig, new):
    o, n, _, width = ref_geometry(orig, new)
    lengths = sorted({1, 5, width - 1, o - 1, 30011, 10 * orig} - {0})
    for L in lengths:
        big = L == 10 * orig
        x = signal(6, L, seed=orig + L)
        want = ref_resample(x, orig, new)
        Lo = want.shape[-1]
        xs = torch.from_numpy(x).cuda()
        cases = [("(2, L)", xs[:2], want[:2])] if big else \
            [("(L,)", xs[0], want[0]), ("(2, L)", xs[:2], want[:2]), ("(3, 2, L)", xs.view(3, 2, L), want.reshape(3, 2, Lo))]
        # rows of a wider buffer at an odd stride (no 16-byte alignment), every other row
        wide = torch.zeros(6, L + 3, device="cuda")
        wide[:, 1:L + 1] = xs
        cases.append(("strided", wide[::2, 1:L + 1], want[::2]))
        for name, inp, ref in cases:
            y = run(inp, orig, new)
            assert y.shape == inp.shape[:-1] + (Lo,) and y.dtype == torch.float32, (name, L)
            err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max()) if Lo else 0.0
            assert err <= 1e-6, (orig, new, L, name, err)


def test_lengths_with_no_output_and_extreme_ratios():
    """L = 0 gives an empty result; a 100:1 downsampling (1,213 taps, input runs past the LDS segment: the kernel's
    global-memory path) and 1 -> 44100 Hz still match the restatement."""
    x = torch.zeros(2, 0, device="cuda")
    assert run(x, 48000, 44100).shape == (2, 0)
    assert run(torch.zeros(2, 1, device="cuda"), 22050, 44100).shape == (2, 2)
    for orig, new, L in ((441000, 4410, 300_007), (1, 44100, 37)):
        xn = signal(2, L, seed=L)
        y = run(torch.from_numpy(xn).cuda(), orig, new).cpu().numpy()
        want = ref_resample(xn, orig, new)
        assert y.shape == want.shape and float(np.abs(y - want).max()) <= 1e-6, (orig, new)


def test_filter_properties():
    """DC gain, a 1 kHz sine at every rate, and the stop band (30 kHz at 96 kHz), on interior samples."""
    def interior(y, k=2000):
        return y[..., k:-k]
    L = 48000
    y = run(torch.ones(L, device="cuda"), 48000, 44100).cpu().numpy()
    assert float(np.abs(interior(y) - 1).max()) < 1e-3
    for orig, _ in RATES[:-1]:
        L = orig                                                       # 1 s
        x = torch.from_numpy(np.sin(2 * np.pi * 1000 * np.arange(L) / orig).astype(np.float32)).cuda()
        y = run(x, orig, MODEL).cpu().numpy().astype(np.float64)
        want = np.sin(2 * np.pi * 1000 * np.arange(y.shape[-1]) / MODEL)
        assert float(np.abs(interior(y - want)).max()) < 2e-3, orig
    x = np.sin(2 * np.pi * 30000 * np.arange(96000) / 96000).astype(np.float32)
    y = run(torch.from_numpy(x).cuda(), 96000, MODEL).cpu().numpy()
    assert float(np.sqrt((interior(y) ** 2).mean()) / np.sqrt((x ** 2).mean())) < 1e-2


def test_full_track_240s_stereo_48k():
    L = 240 * 48000
    x = signal(2, L, seed=240)
    xs = torch.from_numpy(x).cuda()
    y = run(xs, 48000, MODEL)
    assert y.shape == (2, 10_584_000)
    frames = np.r_[0:3, np.linspace(3, 72000 - 4, 300).astype(np.int64), 72000 - 3:72000]    # first, last, 300 between
    want = ref_resample(x, 48000, MODEL, frames=frames)                                  # (2, frames, 147)
    got = y.view(2, -1, 147)[:, torch.from_numpy(frames).cuda()].cpu().numpy()
    assert float(np.abs(got - want).max()) <= 1e-6
    del y
    x7 = np.concatenate([x, x[:, :7]], axis=1)                                           # 11,520,007 samples: rule (b)
    y7 = run(torch.from_numpy(x7).cuda(), 48000, MODEL)
    assert y7.shape == (2, 10_584_006)
    last = ref_resample(x7, 48000, MODEL, frames=np.arange(71995, 72001)).reshape(2, -1)[:, :10_584_006 - 71995 * 147]
    assert float(np.abs(y7[:, 71995 * 147:].cpu().numpy() - last).max()) <= 1e-6


def test_separate_at_48k_is_the_separator_on_resampled_audio():
    from xumx_slicq_amd.inference import separate
    from xumx_slicq_amd.resample import Resample
    from xumx_slicq_amd.separator import seeded_separator
    sep = seeded_separator(realtime=False, wiener=False)
    L = 10 * 48000
    x48 = torch.from_numpy(signal(2, L, seed=48) * 0.5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est, _ = separate(x48, sep, rate=48000, device="cuda")
    assert any("resample to model sample rate" in str(i.message) for i in w)
    x44 = Resample(48000, 44100)(x48.cuda()[None])
    assert x44.shape == (1, 2, 441000)
    direct = sep.to_dict(sep(x44))
    ref44 = torch.from_numpy(ref_resample(x48.numpy(), 48000, MODEL).astype(np.float32)).cuda()[None]
    via_ref = sep.to_dict(sep(ref44))
    for t in est:
        assert torch.equal(est[t], direct[t]), t
        d = est[t] - via_ref[t]
        assert float(d.pow(2).mean().sqrt()) < 1e-4 and float(d.abs().max()) < 1e-3, t


def _write_pcm16(path, x, rate):
    data = np.round(np.clip(x, -1, 1) * 32767).astype("<i2").T.copy().tobytes()
    ch = x.shape[0]
    fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * 2 * ch, 2 * ch, 16)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sI4s", b"RIFF", 4 + 8 + len(fmt) + 8 + len(data), b"WAVE"))
        f.write(struct.pack("<4sI", b"fmt ", len(fmt)) + fmt + struct.pack("<4sI", b"data", len(data)) + data)


def test_cli_on_a_directory_of_mixed_rates(tmp_path):
    from xumx_slicq_amd import audio as A
    from xumx_slicq_amd.inference import inference_main
    files = {"a48f": (48000, signal(2, 52001, 1) * 0.5, "f32"), "b48i": (48000, signal(2, 30011, 2) * 0.5, "pcm16"),
             "c22m": (22050, signal(1, 17000, 3) * 0.5, "pcm16"), "d44": (44100, signal(2, 40000, 4) * 0.5, "f32")}
    (tmp_path / "in").mkdir()
    (tmp_path / "in44").mkdir()
    for name, (rate, x, kind) in files.items():
        for d in ("in",) + (("in44",) if rate == MODEL else ()):
            p = str(tmp_path / d / f"{name}.wav")
            A.save_wav_float(p, torch.from_numpy(x), rate) if kind == "f32" else _write_pcm16(p, x, rate)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inference_main(["--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "piped")])
        inference_main(["--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "serial"), "--serial"])
        inference_main(["--input-dir", str(tmp_path / "in44"), "--output-dir", str(tmp_path / "only44")])
    for name, (rate, x, _) in files.items():
        for t in ("bass", "vocals", "other", "drums"):
            a = (tmp_path / "piped" / name / f"{t}.wav").read_bytes()
            b = (tmp_path / "serial" / name / f"{t}.wav").read_bytes()
            assert a == b and len(a) > 44, (name, t)
            info = A.load_info(str(tmp_path / "piped" / name / f"{t}.wav"))
            assert info["samplerate"] == MODEL and info["channels"] == 2
            assert info["samples"] == ref_length(rate, MODEL, x.shape[-1]), (name, t)
            if rate == MODEL:
                assert a == (tmp_path / "only44" / name / f"{t}.wav").read_bytes(), (name, t)
