"""Host side of the spectrogram (xumx_slicq_amd/visualization.py) and the float64 numpy restatement of its definition
 that tests/test_spectrogram_gpu.py imports as its yardstick.

The restatement is checked here against the reference's own ``overlap_add_slicq`` (tests/golden/spectrogram_mel32.npz,
tools/make_golden_spectrogram.py) and against ``numpy.quantile``; nothing in this file needs a device."""
import struct
import zlib

import numpy as np
import pytest

from conftest import load_golden


# ---- the definition, in float64 numpy -------------------------------------------------------------------------------------
def ref_overlap_add(c, flatten=False):
    """c (..., S, T) complex -> (..., (S + 1) T / 2): ola[p] = sum_i c[i, p - i h]; flatten: (..., S T)."""
    c = np.asarray(c)
    S, T = c.shape[-2:]
    if flatten:
        return c.reshape(*c.shape[:-2], S * T)
    h = T // 2
    out = np.zeros((*c.shape[:-2], (S + 1) * h), dtype=c.dtype)
    for i in range(S):
        out[..., i * h: i * h + T] += c[..., i, :]
    return out


def ref_block_db(c, N, flatten=False):
    """c (B, 2, F, S, T) complex128 -> (B, F, N) float64: overlap-add, 20 log10 |.|, T / 2 columns dropped at each end, the
    mean over the two channels of the dB values, the first N columns."""
    T = c.shape[-1]
    h = T // 2
    ola = ref_overlap_add(c.astype(np.complex128), flatten)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 20.0 * np.log10(np.hypot(ola.real, ola.imag))
        db = db[..., h:]
        db = db[..., :-h]
        db = db.mean(axis=1)
    return db[..., :N]


def ref_block_magnitude(c, N, flatten=False):
    """(B, 2, F, N) float64: the magnitudes behind ``ref_block_db`` (which of them are zero, which are tiny)."""
    h = c.shape[-1] // 2
    ola = ref_overlap_add(c.astype(np.complex128), flatten)
    return np.hypot(ola.real, ola.imag)[..., h:][..., :-h][..., :N]


def ref_columns(blocks, L, n, S, flatten=False):
    """N_b of blocks [(first, F, T)]: min(int((T / L) * n), (S - 1) T / 2), flatten min(..., S T - T)."""
    return [min(int((T / L) * n), S * T - T if flatten else (S - 1) * (T // 2)) for (_, _F, T) in blocks]


def ref_quantile(values, q):
    """(order statistic at floor, at ceil of q (N - 1), their "linear" lerp in float64); -inf counts as a value; equal ends give
    that end and a lower end of -inf gives -inf (numpy's form makes NaN of both)."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    pos = q * (len(v) - 1)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    a, b, t = v[lo], v[hi], pos - lo
    if a == b or np.isneginf(a):
        return a, b, a
    with np.errstate(invalid="ignore"):
        return a, b, (a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t))


def ref_raster_row(db, W):
    """(..., N) -> (..., W), the definition as it reads: pixel w = max of the columns [lo, hi), lo = w N // W,
    hi = max(lo + 1, (w + 1) N // W)."""
    N = db.shape[-1]
    img = np.empty((*db.shape[:-1], W), dtype=db.dtype)
    for w in range(W):
        lo = (w * N) // W
        hi = max(lo + 1, ((w + 1) * N) // W)
        img[..., w] = db[..., lo:hi].max(axis=-1)
    return img


def ref_raster(db_blocks, W):
    """db_blocks: per block (B, F_b, N_b) -> (B, sum F_b, W), ``ref_raster_row`` of every row without the Python loop over
    pixels: with W <= N the ranges tile [0, N) (hi[w] = lo[w + 1]), a reduceat; with W > N every range is one column."""
    rows = []
    for db in db_blocks:
        N = db.shape[-1]
        lo = (np.arange(W, dtype=np.int64) * N) // W
        rows.append(np.maximum.reduceat(db, lo, axis=-1) if W <= N else db[..., lo])
    return np.concatenate(rows, axis=1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype in (np.float64, np.complex128) else np.uint32)


# ---- tests ------------------------------------------------------------------------------------------------------------------
def fixture():
    return load_golden("spectrogram_mel32.npz")


def test_fixture_is_the_mel32_plan_at_n_5000():
    from xumx_slicq_amd.plan import build_plan
    g = fixture()
    p = build_plan("mel", 32, 115.5)
    assert g["x"].shape == (2, 5000) and g["x"].dtype == np.float32
    assert [tuple(r) for r in g["blocks"].tolist()] == p.block_shapes()
    S = p.num_slices(5000)
    for b, (F, T) in enumerate(p.block_shapes()):
        assert g[f"c_{b}"].shape == (2, F, S, T) and g[f"c_{b}"].dtype == np.complex64


@pytest.mark.parametrize("flatten", [False, True])
def test_restated_overlap_add_equals_the_reference(flatten):
    g = fixture()
    for b in range(len(g["blocks"])):
        ours = ref_overlap_add(g[f"c_{b}"].astype(np.complex128), flatten).astype(np.complex64)      # fp32 rounding of float64
        want = g[f"flat_{b}" if flatten else f"ola_{b}"]
        assert ours.shape == want.shape and np.array_equal(ours, want), b


def test_block_columns():
    from xumx_slicq_amd.plan import build_plan
    from xumx_slicq_amd.visualization import block_columns
    for scale, fbins, fmin, ns in (("mel", 32, 115.5, (4 * 1008, 5000, 40000)), ("bark", 262, 32.9, (40000,))):
        p = build_plan(scale, fbins, fmin)
        for n in ns:
            S = p.num_slices(n)
            assert S >= 2
            for flatten in (False, True):
                N = block_columns(p, n, S, flatten)
                assert N == ref_columns(p.blocks, p.L, n, S, flatten)
                most = [S * T - T if flatten else (S - 1) * (T // 2) for (_, _, T) in p.blocks]
                ncoefs = [int((T / p.L) * n) for (_, _, T) in p.blocks]
                assert N == ncoefs and all(a <= m for a, m in zip(N, most)), (n, flatten)          # the truncation decides
                assert min(N) >= 1
    p = build_plan("mel", 32, 115.5)
    assert p.L == 2016
    N = block_columns(p, 5000, p.num_slices(5000))
    assert all(a < (p.num_slices(5000) - 1) * (T // 2) for a, (_, _, T) in zip(N, p.blocks))         # strictly: columns are cut
    assert any(a % 2 for a in N)                                                                    # odd rows exist
    assert block_columns(p, 4 * 1008, 5) == [2 * T for (_, _, T) in p.blocks]
    # a signal longer than its slices hold: the slices decide
    assert block_columns(p, 10 ** 6, 3) == [T for (_, _, T) in p.blocks]
    assert block_columns(p, 10 ** 6, 3, flatten=True) == [2 * T for (_, _, T) in p.blocks]


@pytest.mark.parametrize("N", [1, 2, 39, 525, 4206])
def test_raster_ranges(N):
    from xumx_slicq_amd.visualization import raster_ranges
    for W in sorted({1, 7, max(N - 1, 1), N, N + 1, 4096}):
        lo, hi = raster_ranges(N, W)
        assert lo.dtype == np.int64 and hi.dtype == np.int64 and lo.shape == hi.shape == (W,)
        assert np.all(hi > lo) and np.all(lo >= 0) and np.all(hi <= N)                 # non-empty, in range
        assert np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0)                    # monotone
        assert lo[0] == 0 and hi[-1] == N
        if W <= N:
            assert np.array_equal(hi[:-1], lo[1:])                                      # tile [0, N): no gap, no overlap
        for w in (0, W // 2, W - 1):
            assert lo[w] == (w * N) // W and hi[w] == max(lo[w] + 1, ((w + 1) * N) // W)
    with pytest.raises(ValueError):
        raster_ranges(0, 4)
    # beyond 32 bits
    lo, hi = raster_ranges(3 * 10 ** 9, 4096)
    assert hi[-1] == 3 * 10 ** 9 and lo[4095] == (4095 * 3 * 10 ** 9) // 4096


def test_quantile_restatement_and_host_lerp_equal_numpy():
    from xumx_slicq_amd.visualization import quantile_lerp, quantile_ranks
    rng = np.random.default_rng(7)
    arrays = [rng.standard_normal(n) for n in (1, 2, 3, 10, 1001, 2047, 2049)]
    arrays.append(np.round(rng.standard_normal(500) * 3.0) / 2.0)                       # ties
    arrays.append(np.concatenate([np.full(40, -np.inf), np.round(rng.standard_normal(400) * 4.0)]))   # -inf and ties
    arrays.append(np.array([-np.inf, -np.inf, 1.0, 2.0, 3.0]))                          # q = 0.25, 0.5: a rank at and next to -inf
    for v in arrays:
        for q in (0.0, 0.25, 0.5, 0.999, 1.0):
            a, b, got = ref_quantile(v, q)
            k_lo, k_hi, t = quantile_ranks(len(v), q)
            s = np.sort(v)
            assert (s[k_lo], s[k_hi]) == (a, b)
            assert quantile_lerp(a, b, t) == got and not np.isnan(got)
            with np.errstate(invalid="ignore"):
                want = np.quantile(v, q, method="linear")
            if np.isneginf(a):
                assert got == -np.inf                     # numpy's lerp gives NaN from a lower end of -inf; -inf is meant
            else:
                assert got == want, (len(v), q)
    assert quantile_lerp(-np.inf, -np.inf, 0.3) == -np.inf and quantile_lerp(-np.inf, 1.0, 0.3) == -np.inf
    assert quantile_ranks(1, 0.999) == (0, 0, 0.0)
    with pytest.raises(ValueError):
        quantile_ranks(0, 0.5)
    with pytest.raises(ValueError):
        quantile_ranks(5, 1.5)


def test_restated_db_rules():
    c = np.zeros((1, 2, 1, 3, 4), dtype=np.complex128)
    c[0, 0, 0] = [[1, 2, 3, 4], [10, 20, 30, 40], [100, 200, 300, 400]]
    c[0, 1, 0] = 1.0
    db = ref_block_db(c, 4)
    ola0 = np.array([3 + 10, 4 + 20, 30 + 100, 40 + 200], dtype=np.float64)
    assert np.allclose(db[0, 0], (20 * np.log10(ola0) + 20 * np.log10(2.0)) / 2, rtol=0, atol=1e-12)
    c[0, 1, 0, 0, 2] = -1.0                               # channel 1 cancels at one point: -inf there, whatever channel 0 holds
    assert np.isneginf(ref_block_db(c, 4)[0, 0, 0]) and np.isfinite(ref_block_db(c, 4)[0, 0, 1:]).all()
    flat = ref_block_db(c, 3, flatten=True)
    assert flat.shape == (1, 1, 3) and np.isclose(flat[0, 0, 0], (20 * np.log10(3.0) + 0.0) / 2)
    img = ref_raster([np.arange(12.0).reshape(1, 2, 6), np.arange(3.0).reshape(1, 1, 3)], 3)
    assert img.shape == (1, 3, 3) and img[0, 0].tolist() == [1, 3, 5] and img[0, 2].tolist() == [0, 1, 2]
    assert ref_raster([np.arange(3.0).reshape(1, 1, 3)], 6)[0, 0].tolist() == [0, 0, 1, 1, 2, 2]
    rng = np.random.default_rng(3)
    for N in (1, 2, 39, 525):
        d = rng.standard_normal((2, 3, N)).astype(np.float32)
        d[0, 1, N // 2] = -np.inf
        for W in (1, 7, max(N - 1, 1), N, N + 1, 64, 4096):
            assert np.array_equal(ref_raster([d], W), ref_raster_row(d, W)), (N, W)


def _read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos: pos + 8])
        data = raw[pos + 8: pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n: pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, inter) == (8, 2, 0, 0, 0)
    px = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not px[:, 0].any()                             # filter type 0 on every row
    return px[:, 1:].reshape(h, w, 3)


def test_save_png(tmp_path):
    from xumx_slicq_amd.visualization import colormap, save_png
    img = np.array([[-120.0, -60.0, 0.0, 5.0, -130.0],
                    [-np.inf, np.nan, np.inf, -30.0, -90.0],
                    [0.0, 0.0, 0.0, 0.0, -120.0]], dtype=np.float32)
    for cmap in ("hot", "gray"):
        path = str(tmp_path / f"{cmap}.png")
        save_png(path, img, -120.0, 0.0, cmap)
        px = _read_png(path)
        assert px.shape == (3, 5, 3)
        top, mid, bottom = px[0], px[1], px[2]            # band 0 (low frequencies) is the LAST row of the file
        assert bottom[0].tolist() == [0, 0, 0] and bottom[2].tolist() == [255, 255, 255]            # both end points
        assert bottom[3].tolist() == [255, 255, 255] and bottom[4].tolist() == [0, 0, 0]            # clipped above and below
        assert mid[0].tolist() == mid[1].tolist() == mid[2].tolist() == [0, 0, 0]                    # non-finite: the lowest colour
        assert top[:4].tolist() == [[255, 255, 255]] * 4 and top[4].tolist() == [0, 0, 0]
        want = colormap(cmap, np.array([0.5, 0.75, 0.25]))
        assert bottom[1].tolist() == want[0].tolist() and mid[3].tolist() == want[1].tolist() and mid[4].tolist() == want[2].tolist()
    assert colormap("hot", np.array([0.0, 0.375, 0.75, 1.0])).tolist() == [[0, 0, 0], [255, 0, 0], [255, 255, 0], [255, 255, 255]]
    assert colormap("gray", np.array([0.0, 0.5, 1.0])).tolist() == [[0, 0, 0], [128, 128, 128], [255, 255, 255]]
    # an all-silent picture still writes: vmax = vmin = -inf
    path = str(tmp_path / "silent.png")
    save_png(path, np.full((2, 3), -np.inf, dtype=np.float32), -np.inf, -np.inf)
    assert not _read_png(path).any()
    with pytest.raises(ValueError):
        colormap("inferno", np.zeros(2))
    with pytest.raises(ValueError):
        save_png(path, np.zeros(4), 0.0, 1.0)


def test_band_frequencies():
    from xumx_slicq_amd.plan import build_plan
    from xumx_slicq_amd.visualization import band_frequencies
    for args in (("bark", 262, 32.9), ("mel", 32, 115.5)):
        p = build_plan(*args)
        f = band_frequencies(p)
        assert f.shape == (p.nbands,) and f[0] == 0.0 and f[-1] == 22050.0 and np.all(np.diff(f) > 0)
        assert abs(f[1] - args[2]) < 1e-3
        # the centre bins of the plan are these frequencies rounded to even bins
        assert np.all(np.abs(f * p.L / p.fs - p.c) <= 1.0 + 1e-6)


def test_cli_parser(tmp_path, capsys):
    from xumx_slicq_amd.visualization import parse_args
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    ok = parse_args(["--input-wav", str(wav)])
    assert (ok.sr, ok.cmap, ok.fscale, ok.fbins, ok.fmin, ok.flatten, ok.width, ok.per_block, ok.out_dir) == \
        (44100, "hot", "Bark", 262, 32.9, False, 2560, False, ".")
    full = parse_args(["--input-wav", str(wav), "--sr", "48000", "--cmap", "gray", "--fscale", "mel", "--fbins", "32", "--fmin", "115.5",
                       "--flatten", "--out-dir", str(tmp_path / "o"), "--width", "64", "--per-block"])
    assert (full.sr, full.cmap, full.fscale, full.fbins, full.flatten, full.width, full.per_block) == (48000, "gray", "mel", 32, True, 64, True)
    not_a_dir = tmp_path / "file"
    not_a_dir.write_text("x")
    bad = {"not found": ["--input-wav", str(tmp_path / "missing.wav")],
           "Nyquist": ["--input-wav", str(wav), "--fmin", "4000", "--sr", "8000"],
           "--fmin": ["--input-wav", str(wav), "--fmin", "0"],
           "--sr": ["--input-wav", str(wav), "--sr", "0"],
           "--fbins": ["--input-wav", str(wav), "--fbins", "1"],
           "--width": ["--input-wav", str(wav), "--width", "0"],
           "no directory": ["--input-wav", str(wav), "--out-dir", str(not_a_dir)],
           "--cmap": ["--input-wav", str(wav), "--cmap", "inferno"],
           "--fscale": ["--input-wav", str(wav), "--fscale", "oct"],
           "--input-wav": []}
    for word, argv in bad.items():
        with pytest.raises(SystemExit) as e:
            parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, word


def test_cli_reports_a_plan_that_build_plan_refuses(tmp_path):
    from xumx_slicq_amd.visualization import main
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    with pytest.raises(SystemExit) as e:                  # before the file is read or a device is asked for
        main(["--input-wav", str(wav), "--fscale", "mel", "--fbins", "32", "--fmin", "10.0"])
    assert "no sliCQT plan" in str(e.value) and "reaches across DC" in str(e.value)


def test_cpu_tensors_are_refused():
    import torch
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd import visualization as vis
    from xumx_slicq_amd.transforms import NSGTBase
    base = NSGTBase("mel", 32, 115.5, device="cpu")
    with pytest.raises(_lib.XsqError):
        vis.overlap_add_slicq(torch.zeros(2, 3, 4, 8, dtype=torch.complex64))
    with pytest.raises(_lib.XsqError):
        vis.spectrogram(torch.zeros(1, 2, 5000), base)
    with pytest.raises(_lib.XsqError):
        vis.blockwise_db([torch.zeros(1, 2, F, 6, T, 2) for F, T in base.plan.block_shapes()], 5000, base)
    with pytest.raises(_lib.XsqError):
        vis.order_statistics(torch.zeros(1, 8), 0.5)


def test_entry_points_refuse_bad_geometry_without_a_device():
    import ctypes as C
    from xumx_slicq_amd import _lib
    F = np.array([1], dtype=np.int32)
    T = np.array([18], dtype=np.int32)
    N = np.array([4], dtype=np.int32)
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    rc = _lib.lib.xsq_spectrogram_db(1, F.ctypes.data, T.ctypes.data, N.ctypes.data, p, 1, 3, 0, p, None)
    assert rc < 0 and "multiple of 4" in _lib.last_error()
    T[0] = 16
    N[0] = 17                                             # (S - 1) h = 16
    rc = _lib.lib.xsq_spectrogram_db(1, F.ctypes.data, T.ctypes.data, N.ctypes.data, p, 1, 3, 0, p, None)
    assert rc < 0 and "hold 16" in _lib.last_error()
    N[0] = 0
    rc = _lib.lib.xsq_spectrogram_raster(1, F.ctypes.data, N.ctypes.data, p, 1, 8, p, None)
    assert rc < 0 and "too short" in _lib.last_error()
    N[0] = 4
    rc = _lib.lib.xsq_spectrogram_order_stats(1, F.ctypes.data, N.ctypes.data, p, 1, 2, 4, p, p, 1 << 20, None)
    assert rc < 0 and "ranks" in _lib.last_error()
    rc = _lib.lib.xsq_spectrogram_order_stats(1, F.ctypes.data, N.ctypes.data, p, 1, 2, 3, p, p, 16, None)
    assert rc < 0 and "workspace" in _lib.last_error()
    many = np.full(_lib.lib.xsq_spectrogram_max_blocks() + 1, 4, dtype=np.int32)
    rc = _lib.lib.xsq_spectrogram_overlap_add(len(many), many.ctypes.data, many.ctypes.data, p, 1, 2, 0, p, None)
    assert rc < 0 and "blocks" in _lib.last_error()
    assert _lib.lib.xsq_spectrogram_overlap_add_size(1, F.ctypes.data, T.ctypes.data, 2, 6, 0) == 2 * 2 * 1 * 7 * 8
    assert _lib.lib.xsq_spectrogram_overlap_add_size(1, F.ctypes.data, T.ctypes.data, 2, 6, 1) == 2 * 2 * 1 * 6 * 16
