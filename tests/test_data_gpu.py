"""``xsq_batch_assemble`` (csrc/batch.hip) against a numpy fp32 restatement of its contract, BITWISE: every batch of a
table that walks the alignment cases of source and destination rows, in both storages, with sentinel margins around the
output buffers.  Every index in these tables is in range: no test feeds the kernel a bad table."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SOURCES = ("vocals", "drums", "bass", "other")
TOC = (1, 3, 0, 2)                       # target plane (bass, vocals, other, drums) of each source column
GAINS = (np.float32(0.25), np.float32(1.0), np.nextafter(np.float32(1.25), np.float32(0)))
SENTINEL = np.float32(-12345.678)


def restate(rows, lengths, rec, n):
    """Section "Arithmetic" of the contract: rows[t] is the (8, len) fp32 image of track t, rec one step's (B, 4, 4)
    records.  Products are rounded to fp32 before the sequential fp32 sums."""
    B = rec.shape[0]
    x, y = np.zeros((B, 2, n), np.float32), np.zeros((4, B, 2, n), np.float32)
    for b in range(B):
        for s in range(4):
            t, start, swap = int(rec[b, s, 0]), int(rec[b, s, 1]), int(rec[b, s, 3])
            gain = rec[b, s, 2:3].view(np.float32)[0]
            for c in range(2):
                v = np.zeros(n, np.float32)
                seg = rows[t][2 * s + (c ^ swap), start:start + n]           # nothing at or past len: zeros
                v[:len(seg)] = seg
                ys = (gain * v).astype(np.float32)
                y[TOC[s], b, c] = ys
                x[b, c] = ys if s == 0 else (x[b, c] + ys).astype(np.float32)
    return x, y


def lengths_for(n):
    # n + 37, n - 5 (shorter than the excerpt: its tail is zero; at n < 6 the shortest track there is, one sample), 3n + 1
    return [n + 37, max(n - 5, 1), 3 * n + 1]


@functools.lru_cache(maxsize=None)
def pcm_tracks(n):
    rng = np.random.default_rng(1000 + n)
    return [{s: rng.integers(-32768, 32768, size=(2, ln), dtype=np.int16) for s in SOURCES} for ln in lengths_for(n)]


@functools.lru_cache(maxsize=None)
def float_tracks(n):
    rng = np.random.default_rng(2000 + n)
    return [{s: rng.standard_normal((2, ln)).astype(np.float32) * np.float32(0.3) for s in SOURCES} for ln in lengths_for(n)]


def images(tracks):
    return [np.concatenate([np.asarray(tr[s], np.float32) / (np.float32(32768) if tr[s].dtype == np.int16 else np.float32(1))
                            for s in SOURCES], axis=0) for tr in tracks]


@functools.lru_cache(maxsize=None)
def records(n, B):
    """Items whose columns walk: track 0 at starts 0 .. 7 (every residue mod 8), 8 + r for more, and len - n = 37 exactly;
    the short track at 0; track 2 at 0, at len - n = 2n + 1 exactly and at odd places between; all three gains, both swaps;
    item 0 has all four columns on track 2.  Padded by whole items to one more than a multiple of B: the last batch is ragged
    for B > 1."""
    L = lengths_for(n)
    combos = [(0, st) for st in list(range(8)) + [13, 22, 37]] + [(1, 0)] + \
             [(2, st) for st in sorted({0, 2 * n + 1, min(3, 2 * n + 1), min(n + 2, 2 * n + 1), min(6, 2 * n + 1), 2 * n})]
    for t, st in combos:
        assert 0 <= st and (st + n <= L[t] or (L[t] < n and st == 0)), (t, st)
    items = []
    nitems = len(combos)
    while nitems % B != 1 % B:
        nitems += 1
    for i in range(nitems):
        item = []
        for s in range(4):
            t, st = combos[(i + 5 * s) % len(combos)]
            if i == 0:
                t, st = 2, (0, 2 * n + 1, n, 1)[s]
            gain = GAINS[(i + s) % 3]
            item.append([t, st, int(np.asarray(gain, np.float32).view(np.int32)), (i + (s >> 1) + (i >> 2)) & 1])
        items.append(item)
    rec = np.asarray(items, dtype=np.int32)
    assert {0, 1} == set(rec[..., 3].ravel().tolist()) and len(set(rec[0, :, 0].tolist())) == 1
    assert {st % 8 for st in rec[..., 1].ravel().tolist()} == set(range(8)) or n == 1
    return rec


def dataset(n, storage):
    from xumx_slicq_amd.data import DeviceDataset
    tracks = pcm_tracks(n) if storage == "pcm16" else float_tracks(n)
    return DeviceDataset.from_arrays(tracks, storage=storage, device="cuda"), images(tracks)


def guarded(shape, margin):
    """A contiguous fp32 view of ``shape`` with ``margin`` sentinel floats on either side."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * margin,), float(SENTINEL), dtype=torch.float32, device="cuda")
    return buf, buf[margin:margin + numel].view(*shape)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("storage", ["pcm16", "fp32"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 7, 1000, 9031])
def test_batches_equal_the_restatement_bitwise(n, B, storage):
    """Every step of the table (the kernel's ``step`` argument runs from 0 up; the ragged last batch starts where the full
    ones end), into buffers that start on a 16-byte boundary (margin 64) and off one (margin 61: with odd n every row of x
    and y then has its own alignment)."""
    ds, rows = dataset(n, storage)
    rec = records(n, B)
    table = ds.table(rec, B, n)
    assert table.nsteps >= 2 and table.items_of(table.nsteps - 1) == 1
    for step in range(table.nsteps):
        Bk = table.items_of(step)
        want_x, want_y = restate(rows, ds.lengths, rec[step * B:step * B + Bk], n)
        for margin in (64, 61):
            xbuf, x = guarded((Bk, 2, n), margin)
            ybuf, y = guarded((4, Bk, 2, n), margin)
            got = ds.batch(table, step, out=(x, y))
            assert got[0] is x and got[1] is y
            torch.cuda.synchronize()
            assert same_bits(x.cpu().numpy(), want_x), (step, margin, "x")
            assert same_bits(y.cpu().numpy(), want_y), (step, margin, "y")
            for buf in (xbuf, ybuf):
                edge = torch.cat([buf[:margin], buf[-margin:]]).cpu().numpy()
                assert (edge == SENTINEL).all(), (step, margin, "sentinel")


def test_the_restatement_rounds_the_product_before_the_sums():
    """What the bitwise test above can tell apart: on its own data a fused multiply-add in the mix differs from the
    contract's rounded product in some sample (pure numpy, float64 standing in for the unrounded product)."""
    n = 1000
    rows = images(float_tracks(n))
    rec = next(r[None] for r in records(n, 1) if 1 not in r[:, 0])           # an item without the short track
    x, y = restate(rows, lengths_for(n), rec, n)
    g = np.ascontiguousarray(rec[0, :, 2]).view(np.float32).astype(np.float64)
    v = [rows[int(rec[0, s, 0])][2 * s + int(rec[0, s, 3]), int(rec[0, s, 1]):int(rec[0, s, 1]) + n].astype(np.float64) for s in range(4)]
    fused = (g[0] * v[0]).astype(np.float32)
    for s in range(1, 4):
        fused = (fused.astype(np.float64) + g[s] * v[s]).astype(np.float32)
    assert not same_bits(fused, x[0, 0])


@pytest.mark.parametrize("n", [7, 1000])
def test_pcm16_and_fp32_pools_of_the_same_values_give_identical_batches(n):
    from xumx_slicq_amd.data import DeviceDataset
    tracks = pcm_tracks(n)
    a = DeviceDataset.from_arrays(tracks, storage="pcm16", device="cuda")
    b = DeviceDataset.from_arrays(tracks, storage="fp32", device="cuda")
    rec = records(n, 3)
    ta, tb = a.table(rec, 3, n), b.table(rec, 3, n)
    for step in range(ta.nsteps):
        (xa, ya), (xb, yb) = a.batch(ta, step), b.batch(tb, step)
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ya.view(torch.int32), yb.view(torch.int32))


def test_owned_buffers_keep_the_last_five_batches_intact():
    n, B = 1000, 3
    ds, rows = dataset(n, "pcm16")
    rec = np.concatenate([records(n, B)[:18]] * 2)
    table = ds.table(rec, B, n)
    out = [ds.batch(table, k) for k in range(6)]
    assert len({x.data_ptr() for x, _ in out[:5]}) == 5 and out[5][0].data_ptr() == out[0][0].data_ptr()
    for k in range(1, 6):                                      # batch 0's buffers now hold batch 5; 1 .. 4 are untouched
        want_x, want_y = restate(rows, ds.lengths, rec[k * B:(k + 1) * B], n)
        assert same_bits(out[k][0].cpu().numpy(), want_x) and same_bits(out[k][1].cpu().numpy(), want_y)


@pytest.mark.parametrize("storage", ["pcm16", "fp32"])
def test_pieces_concatenate_to_the_stems_and_their_fp32_sum(storage):
    n = 1000
    ds, rows = dataset(n, storage)
    for i, chunk in ((2, 1000), (0, 256), (1, 5000), (2, 9031)):
        length = int(ds.lengths[i])
        got = [(x.clone(), y.clone()) for x, y in ds.pieces(i, chunk)]
        assert [x.shape[-1] for x, _ in got] == [min(chunk, length - s) for s in range(0, length, chunk)]
        assert all(x.shape[:2] == (1, 2) and y.shape[:3] == (4, 1, 2) for x, y in got)
        x = torch.cat([x for x, _ in got], dim=-1)[0].cpu().numpy()
        y = torch.cat([y for _, y in got], dim=-1)[:, 0].cpu().numpy()
        stems = rows[i].reshape(4, 2, length)
        mix = ((stems[0] + stems[1]) + stems[2]) + stems[3]
        assert same_bits(x, mix)
        for s in range(4):
            assert same_bits(y[TOC[s]], stems[s])
