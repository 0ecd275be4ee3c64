"""Host side of the device-resident dataset (xumx_slicq_amd/data.py; MUSDBDataset of data.py:211-393 in the reference's
training configuration): the epoch's draw table, its validation, the constructors and the pool layout, and the argument
checks of ``xsq_batch_assemble``.  No GPU: pools are built on the CPU, where they can be inspected but not sampled."""
import os
import wave

import numpy as np
import pytest

from xumx_slicq_amd import data as D

SOURCES = ("vocals", "drums", "bass", "other")


def _tracks(lengths, seed=3):
    rng = np.random.default_rng(seed)
    return [{s: rng.integers(-32768, 32768, size=(2, n), dtype=np.int16) for s in SOURCES} for n in lengths]


@pytest.fixture(scope="module")
def ds():
    return D.DeviceDataset.from_arrays(_tracks([50000, 30011, 44100 * 3, 7]), storage="pcm16", device="cpu")


def test_draw_epoch_is_deterministic_in_seed_and_epoch(ds):
    a = ds.draw_epoch(42, 1, batch_size=16, seq_dur=0.5, samples_per_track=8)
    b = ds.draw_epoch(42, 1, batch_size=16, seq_dur=0.5, samples_per_track=8)
    assert a.records.dtype == np.int32 and np.array_equal(a.records, b.records)
    assert not np.array_equal(a.records, ds.draw_epoch(42, 2, 16, 0.5, 8).records)
    assert not np.array_equal(a.records, ds.draw_epoch(43, 1, 16, 0.5, 8).records)
    # pinned: numpy's PCG64 stream is the same on every machine
    first = ds.draw_epoch(42, 1, 16, 0.5, 8).records[0, :, 0].tolist()
    want = np.random.default_rng([42, 1]).integers(0, 4, size=(32, 4))[0].tolist()
    assert first == want


def test_item_and_batch_counts_include_the_ragged_last_batch(ds):
    t = ds.draw_epoch(1, 1, batch_size=5, seq_dur=0.25, samples_per_track=3)
    assert (t.nitems, t.nsteps, len(t), t.n) == (12, 3, 3, 11025)
    assert [t.items_of(k) for k in range(3)] == [5, 5, 2]
    with pytest.raises(IndexError):
        t.items_of(3)
    t = ds.draw_epoch(1, 1, batch_size=4, seq_dur=0.25, samples_per_track=3)
    assert t.nsteps == 3 and t.items_of(2) == 4
    assert ds.draw_epoch(1, 1, 32, 2.0).nitems == 4 * 64                  # the reference's 64 samples per track


def test_starts_gains_and_swaps_are_in_range(ds):
    t = ds.draw_epoch(7, 3, batch_size=8, seq_dur=0.75, samples_per_track=200)
    n = t.n
    assert n == 33075
    track, start, swap = t.records[..., 0], t.records[..., 1], t.records[..., 3]
    ln = ds.lengths[track]
    assert track.min() == 0 and track.max() == 3
    assert (start >= 0).all() and (np.where(ln >= n, start + n <= ln, start == 0)).all()
    assert (start[ln < n] == 0).all() and (ln < n).any()                   # tracks 1 and 3 are shorter than the excerpt
    long = track == 2
    assert start[long].max() > (44100 * 3 - n) * 0.9 and start[long].min() < (44100 * 3 - n) * 0.1
    g = t.gains
    assert g.dtype == np.float32 and (g >= np.float32(0.25)).all() and (g < np.float32(1.25)).all()
    assert g.min() < 0.3 and g.max() > 1.2
    assert set(np.unique(swap).tolist()) == {0, 1} and 0.4 < swap.mean() < 0.6


def test_the_largest_gain_draw_stays_below_the_upper_bound():
    k = np.float32((1 << 23) - 1)
    assert np.float32(0.25) + k * np.float32(2.0 ** -23) < np.float32(1.25)


def test_every_track_is_reachable_over_a_few_epochs(ds):
    seen = set()
    for epoch in range(1, 4):
        seen |= set(np.unique(ds.draw_epoch(0, epoch, 4, 0.1, samples_per_track=4).records[..., 0]).tolist())
    assert seen == {0, 1, 2, 3}


def test_augment_off_gives_unit_gain_and_no_swap(ds):
    t = ds.draw_epoch(42, 1, 16, 0.5, 8, augment=False)
    assert (t.gains == np.float32(1.0)).all() and (t.records[..., 3] == 0).all()
    on = ds.draw_epoch(42, 1, 16, 0.5, 8)
    assert np.array_equal(t.records[..., :2], on.records[..., :2])         # tracks and starts are drawn first


def test_table_validation_refuses_a_bad_record(ds):
    good = ds.draw_epoch(5, 1, 4, 0.5, 2).records
    n = 22050
    D.validate_table(good, ds.lengths, n)
    for field, value, where in ((0, 4, "track"), (0, -1, "track"), (1, -1, "reads"), (1, 50000 - n + 1, "reads"), (3, 2, "swap")):
        bad = good.copy()
        bad[1, 2, 0] = 0                                                   # a track of 50000 samples
        bad[1, 2, 1] = 0
        bad[1, 2, field] = value
        with pytest.raises(ValueError, match=where):
            D.validate_table(bad, ds.lengths, n)
        with pytest.raises(ValueError, match=where):
            ds.table(bad, 4, n)
    bad = good.copy()
    bad[0, 0, 0], bad[0, 0, 1] = 3, 1                                      # the 7-sample track must start at 0
    with pytest.raises(ValueError, match="reads"):
        D.validate_table(bad, ds.lengths, n)
    bad = good.copy()
    bad[0, 0, 2] = np.float32(np.inf).view(np.int32)
    with pytest.raises(ValueError, match="finite"):
        D.validate_table(bad, ds.lengths, n)
    with pytest.raises(ValueError, match="int32"):
        D.validate_table(good.astype(np.int64), ds.lengths, n)


def test_from_arrays_storage_rules():
    tr = _tracks([100, 37])
    with pytest.raises(ValueError, match="quantised"):
        D.DeviceDataset.from_arrays([{s: v.astype(np.float32) / 32768 for s, v in t.items()} for t in tr], storage="pcm16", device="cpu")
    with pytest.raises(ValueError, match="other"):
        D.DeviceDataset.from_arrays([{s: tr[0][s] for s in SOURCES[:3]}], device="cpu")
    with pytest.raises(ValueError, match="storage"):
        D.DeviceDataset.from_arrays(tr, storage="fp16", device="cpu")
    p16 = D.DeviceDataset.from_arrays(tr, storage="pcm16", device="cpu")
    p32 = D.DeviceDataset.from_arrays(tr, storage="fp32", device="cpu")
    assert p16.pool.dtype.is_floating_point is False and p32.pool.dtype.is_floating_point
    assert np.array_equal(p16.pool.numpy().astype(np.float32) / np.float32(32768), p32.pool.numpy())
    assert p16.sources == SOURCES and p16.target_of_column == (1, 3, 0, 2)
    from xumx_slicq_amd.separator import Separator
    assert [Separator.sources[t] for t in p16.target_of_column] == list(SOURCES)
    # the pool's layout: 8 rows per track, stride rounded up to 8, zero padding
    assert p16.lengths.tolist() == [100, 37] and p16.offsets.tolist() == [0, 8 * 104] and p16.pool.numel() == 8 * (104 + 40)
    rows = p16.pool[8 * 104:].view(8, 40).numpy()
    for s, name in enumerate(SOURCES):
        for c in range(2):
            assert np.array_equal(rows[2 * s + c, :37], tr[1][name][c]) and not rows[2 * s + c, 37:].any()
    assert p16.tracks.tolist() == [[0, 100], [8 * 104, 37]]


def _write_wav(path, frames, rate=44100):
    """frames int16 (samples, channels)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(frames.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(frames).astype("<i2").tobytes())


def test_from_directory_reads_the_musdb_layout(tmp_path):
    rng = np.random.default_rng(11)
    lengths = {"b song": 45, "a song": 16, "c song": 9}
    audio = {}
    for name, n in lengths.items():
        for s in SOURCES:
            ch = 1 if (name == "c song" and s == "drums") else 2            # one mono stem
            audio[name, s] = rng.integers(-32768, 32768, size=(n, ch), dtype=np.int16)
            _write_wav(str(tmp_path / name / (s + ".wav")), audio[name, s])
    (tmp_path / "not a track").mkdir()
    for storage in ("pcm16", "fp32"):
        ds = D.DeviceDataset.from_directory(str(tmp_path), storage=storage, device="cpu")
        assert ds.names == ["a song", "b song", "c song"] and ds.lengths.tolist() == [16, 45, 9]
        assert ds.offsets.tolist() == [0, 8 * 16, 8 * 16 + 8 * 48] and ds.pool.numel() == 8 * (16 + 48 + 16)
        for t, name in enumerate(ds.names):
            n, st = lengths[name], (lengths[name] + 7) // 8 * 8
            rows = ds.pool[int(ds.offsets[t]):int(ds.offsets[t]) + 8 * st].view(8, st).numpy()
            for s, src in enumerate(SOURCES):
                a = audio[name, src]
                for c in range(2):
                    want = a[:, min(c, a.shape[1] - 1)]                      # mono is duplicated
                    want = want if storage == "pcm16" else want.astype(np.float32) / np.float32(32768)
                    assert np.array_equal(rows[2 * s + c, :n], want), (storage, name, src, c)
                    assert not rows[2 * s + c, n:].any()
    sub = D.DeviceDataset.from_directory(str(tmp_path), names=["c song", "a song"], device="cpu")
    assert sub.names == ["c song", "a song"] and sub.lengths.tolist() == [9, 16]
    _write_wav(str(tmp_path / "d song" / "vocals.wav"), audio["a song", "vocals"], rate=48000)
    for s in SOURCES[1:]:
        _write_wav(str(tmp_path / "d song" / (s + ".wav")), audio["a song", s])
    with pytest.raises(ValueError, match="sample rate"):
        D.DeviceDataset.from_directory(str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="unequal"):
        _write_wav(str(tmp_path / "d song" / "vocals.wav"), audio["b song", "vocals"])
        D.DeviceDataset.from_directory(str(tmp_path), names=["d song"], device="cpu")


def test_a_cpu_pool_builds_no_batches(ds):
    from xumx_slicq_amd import _lib
    t = ds.draw_epoch(1, 1, 2, 0.1, 1)
    with pytest.raises(_lib.XsqError, match="ROCm"):
        ds.batch(t, 0)


def test_batch_assemble_entry_point_is_declared_exported_and_checks_its_arguments():
    from conftest import ROOT
    from xumx_slicq_amd import _lib
    assert hasattr(_lib.lib, "xsq_batch_assemble") and "xsq_batch_assemble" in _lib.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    assert "int xsq_batch_assemble(" in hdr and "data.py:316-390" in hdr
    assert "batch.hip" in open(os.path.join(ROOT, "xumx_slicq_amd", "csrc", "Makefile")).read()
    assert _lib.lib.xsq_abi_version() == 2                                  # an additive entry point
    f = _lib.lib.xsq_batch_assemble
    # argument checks run on the host: no device memory is touched (the pointers are never dereferenced)
    p = 4096
    assert f(None, 0, None, 1, None, 0, 1, 10, None, None, None, None) < 0 and "null" in _lib.last_error()
    for missing in range(6):
        ptrs = [p] * 6
        ptrs[missing] = None
        pool, tracks, draws, toc, x, y = ptrs
        assert f(pool, 0, tracks, 1, draws, 0, 1, 10, toc, x, y, None) < 0 and "null" in _lib.last_error()
    good = dict(dtype=0, ntracks=1, step=0, B=1, n=10)
    for key, value in (("dtype", 2), ("dtype", -1), ("ntracks", 0), ("step", -1), ("B", 0), ("B", -3), ("n", 0), ("n", 2 ** 31)):
        a = dict(good, **{key: value})
        assert f(p, a["dtype"], p, a["ntracks"], p, a["step"], a["B"], a["n"], p, p, p, None) < 0, (key, value)
        assert "xsq_batch_assemble" in _lib.last_error()
