"""The spectrogram on the device (xumx_slicq_amd/visualization.py, csrc/spectrogram.hip) against the reference's own
overlap-add (tests/golden/spectrogram_mel32.npz), against the float64 restatement of tests/test_spectrogram_cpu.py, and against
itself where indexing goes wrong.

Shapes, the smallest that reach every index path: Mel-32 (slice length 2016, 23 blocks, 9 + 2 + 2 bands in multi-band blocks)
with n = 4032 (every N_b = (S - 1) h_b exactly, all even) and n = 5000 (N_b cut short, most of them odd: the last 16-byte group
of a row is half used), B = 1 and 2; Mel-32 with n = 40000 (rows of up to 4206 columns: three workgroups per row in the dB pass,
two histogram workgroups per block); Bark-262 with n = 40000 (70 blocks, the one-band DC block included).

dB rule (oracle/parity.py): e_gpu <= M * E in absolute dB over the finite points, both errors against the float64 restatement
fed the SAME device coefficients; E = the largest error over the blocks of an fp32 torch-CPU restatement of the same steps.
Points whose float64 magnitude is nonzero but below 2^-100 would be left out; the test asserts they are under 1e-3 of all points
(there are none for these inputs: seeded Gaussian noise of seeds SEED + n + B, i.e. 5033, 5034, 6001, 6002, 41001 -- for each of
them the CPU oracle's forward, oracle.slicqt.forward on Mel-32 and, for 41001, on Bark-262, was checked to give no such point;
its only exact zeros are one to three points of the flattened layout at n = 40000, in the padding behind the signal).  M: the smallest power of two at least twice the worst ratio measured on MI355X
(profiles/spectrogram_parity.json), never above M_CAP.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle.parity import M_CAP, Tables
from test_spectrogram_cpu import bits, ref_block_db, ref_block_magnitude, ref_columns, ref_quantile, ref_raster

pytestmark = pytest.mark.gpu

PLANS = {"mel": ("mel", 32, 115.5), "bark": ("bark", 262, 32.9)}
CASES = [("mel", 4032, 1), ("mel", 4032, 2), ("mel", 5000, 1), ("mel", 5000, 2), ("mel", 40000, 1), ("bark", 40000, 1)]
SEED = 1000
TINY = 2.0 ** -100
# worst e_gpu / E measured on MI355X (profiles/spectrogram_parity.json): db 1.62 (mel n=4032 B=1, block 22), db-flatten 1.53
# (mel n=5000 B=1, block 14) -> the smallest power of two at least twice the worst is 4 for both
M = {"spectrogram/db": 4, "spectrogram/db-flatten": 4}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
TABLES = Tables("spectrogram_parity", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    TABLES.dump()


@functools.lru_cache(maxsize=None)
def base_of(pk):
    from xumx_slicq_amd.transforms import NSGTBase
    return NSGTBase(*PLANS[pk], device="cuda")


def noise(n, B, kind="noise"):
    g = torch.Generator().manual_seed(SEED + n + B)
    x = 0.1 * torch.randn(B, 2, n, generator=g)
    if kind == "silent":
        x.zero_()
    elif kind == "half":
        x[:, 1] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def forward_of(pk, n, B, kind="noise"):
    """(audio on the device, the block list NSGT_SL returns, the same blocks on the host as complex64 (B, 2, F, S, T))."""
    from xumx_slicq_amd.transforms import NSGT_SL
    x = noise(n, B, kind).cuda()
    with torch.no_grad():
        X = NSGT_SL(base_of(pk))(x)
    host = [torch.view_as_complex(b.cpu().contiguous()).numpy() for b in X]
    return x, X, host


@functools.lru_cache(maxsize=None)
def ref_db_of(pk, n, B, flatten, kind="noise"):
    """Per block: (float64 restatement (B, F, N), float64 magnitudes (B, 2, F, N)) from the device's coefficients."""
    _, _, host = forward_of(pk, n, B, kind)
    plan = base_of(pk).plan
    N = ref_columns(plan.blocks, plan.L, n, plan.num_slices(n), flatten)
    return [(ref_block_db(c, Nb, flatten), ref_block_magnitude(c, Nb, flatten)) for c, Nb in zip(host, N)]


def cpu32_db(c, N, flatten):
    """The same steps in fp32 torch on the CPU, as the reference writes them (visualization.py:13-35, :61-81)."""
    c = torch.from_numpy(c)                                   # (B, 2, F, S, T) complex64
    S, T = c.shape[-2:]
    h = T // 2
    if flatten:
        ola = torch.flatten(c, start_dim=-2, end_dim=-1)
    else:
        ola = torch.zeros((*c.shape[:-2], (S + 1) * h), dtype=c.dtype)
        for i in range(S):
            ola[..., i * h: i * h + T] += c[..., i, :]
    mls = 20.0 * torch.log10(torch.abs(ola))
    mls = mls[..., h:][..., :-h]
    return torch.mean(mls, dim=1)[..., :N].numpy()


def device_db(pk, n, B, flatten, kind="noise"):
    from xumx_slicq_amd.visualization import blockwise_db
    _, X, _ = forward_of(pk, n, B, kind)
    return [d.cpu().numpy() for d in blockwise_db(X, n, base_of(pk), flatten=flatten)]


# ---- overlap-add -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flatten", [False, True])
def test_overlap_add_is_bit_for_bit_the_reference(flatten):
    from xumx_slicq_amd.visualization import overlap_add_blocks, overlap_add_slicq
    g = load_golden("spectrogram_mel32.npz")
    nb = len(g["blocks"])
    outs = []
    for b in range(nb):
        c = torch.from_numpy(g[f"c_{b}"]).cuda()                                        # the reference's coefficients as they are
        got = overlap_add_slicq(c, flatten=flatten)
        want = g[f"flat_{b}" if flatten else f"ola_{b}"]
        assert got.dtype == torch.complex64 and tuple(got.shape) == want.shape
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), b
        real = overlap_add_slicq(torch.view_as_real(c), flatten=flatten)                # the real view gives the real view
        assert real.dtype == torch.float32 and tuple(real.shape) == (*want.shape, 2)
        assert np.array_equal(bits(real.cpu().numpy()).reshape(bits(want).shape), bits(want))
        outs.append(want)
    # every block in one launch over an arena, a leading batch dimension in front: the same bits
    arena_blocks = [torch.view_as_real(torch.from_numpy(np.stack([g[f"c_{b}"], g[f"c_{b}"][::-1]])).contiguous()) for b in range(nb)]
    arena = torch.cat([a.reshape(-1) for a in arena_blocks]).cuda()
    views = base_of("mel").nsgt.table.views(arena, (2, 2), arena_blocks[0].shape[3])
    for b, v in enumerate(overlap_add_blocks(views, base_of("mel"), flatten=flatten)):
        got = torch.view_as_complex(v).cpu().numpy()
        assert np.array_equal(bits(got[0]), bits(outs[b])) and np.array_equal(bits(got[1]), bits(outs[b][::-1].copy())), b


# ---- dB ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flatten", [False, True])
@pytest.mark.parametrize("pk,n,B", CASES)
def test_db_against_float64(pk, n, B, flatten):
    plan = base_of(pk).plan
    _, _, host = forward_of(pk, n, B)
    got = device_db(pk, n, B, flatten)
    ref = ref_db_of(pk, n, B, flatten)
    e_gpu, e_cpu, labels, points, tiny = [], [], [], 0, 0
    for k, (c, d, (want, mag)) in enumerate(zip(host, got, ref)):
        assert d.shape == want.shape == (B, plan.blocks[k][1], want.shape[-1]) and d.dtype == np.float32
        zero = (mag == 0.0).any(axis=1)
        assert np.array_equal(np.isneginf(d), zero) and np.array_equal(np.isneginf(want), zero), k       # -inf exactly where a channel is 0
        small = ((mag != 0.0) & (mag < TINY)).any(axis=1)
        keep = ~zero & ~small
        assert np.isfinite(d[keep]).all()
        points += d.size
        tiny += int(small.sum())
        cpu = cpu32_db(c, want.shape[-1], flatten)
        e_gpu.append(float(np.abs(d[keep] - want[keep]).max()) if keep.any() else 0.0)
        e_cpu.append(float(np.abs(cpu[keep] - want[keep]).max()) if keep.any() else 0.0)
        labels.append(f"block {k} T={plan.blocks[k][2]}")
    assert tiny < 1e-3 * points
    stage = "spectrogram/db-flatten" if flatten else "spectrogram/db"
    bad, worst = TABLES.judge(stage, f"{pk} n={n} B={B}", (e_gpu, e_gpu), (e_cpu, e_cpu), labels)
    print(f"{stage} {pk} n={n} B={B}: worst e_gpu / E = {worst:.3f}, e_gpu max {max(e_gpu):.3e} dB, E {max(e_cpu):.3e} dB")
    assert not bad, bad


def test_columns_span_the_signal():
    from xumx_slicq_amd.visualization import block_columns
    plan = base_of("mel").plan
    for n in (4032, 5000):
        S = plan.num_slices(n)
        got = device_db("mel", n, 1, False)
        assert [d.shape[-1] for d in got] == block_columns(plan, n, S) == ref_columns(plan.blocks, plan.L, n, S)


# ---- order statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 2047, 2049, 9001])
def test_order_statistics_are_exact(N):
    from xumx_slicq_amd.visualization import order_statistics, quantile, quantile_ranks
    rng = np.random.default_rng(N)
    v = np.stack([(rng.integers(-40, 40, N) / 4.0).astype(np.float32), rng.standard_normal(N).astype(np.float32) * 1e-3])
    v[0, rng.integers(0, N, max(N // 8, 1))] = -np.inf                                  # ties and -inf in row 0
    if N > 2:
        v[1, 0], v[1, 1] = np.inf, -np.inf
    dev = torch.from_numpy(v).cuda()
    for q in (0.0, 0.5, 0.999, 1.0):
        stats, t = order_statistics(dev, q)
        k_lo, k_hi, t_want = quantile_ranks(N, q)
        assert t == t_want and stats.dtype == np.float32 and stats.shape == (2, 2)
        for r in range(2):
            s = np.sort(v[r])
            assert np.array_equal(bits(stats[r]), bits(np.array([s[k_lo], s[k_hi]]))), (q, r)
            assert quantile(dev, q)[r] == ref_quantile(v[r], q)[2]


@pytest.mark.parametrize("q", [0.5, 0.999, 1.0])
def test_vmax_is_the_quantile_of_the_full_resolution_db_values(q):
    from xumx_slicq_amd.visualization import spectrogram
    for pk, n, B in (("mel", 5000, 2), ("mel", 40000, 1)):
        x, _, _ = forward_of(pk, n, B)
        sp = spectrogram(x, base_of(pk), width=7, q=q, per_block=True)
        db = device_db(pk, n, B, False)
        for b in range(B):
            a, c, want = ref_quantile(np.concatenate([d[b].reshape(-1) for d in db]), q)
            assert sp.vmax[b] == want and sp.vmin[b] == want - 120.0, (pk, n, b)
        for k, d in enumerate(db):                                                       # the reference's per-block scale
            assert np.array_equal(bits(sp.blocks[k].cpu().numpy()), bits(d))
            for b in range(B):
                assert sp.block_vmax[k, b] == ref_quantile(d[b], q)[2], (k, b)


# ---- raster and the whole call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pk,n,B", [("mel", 5000, 2), ("mel", 40000, 1), ("bark", 40000, 1)])
def test_image_is_the_raster_of_blockwise_db(pk, n, B):
    from xumx_slicq_amd.visualization import band_frequencies, spectrogram
    base = base_of(pk)
    x, _, _ = forward_of(pk, n, B)
    for flatten in (False, True):
        db = device_db(pk, n, B, flatten)
        for W in (1, 7, 64, 4096):
            sp = spectrogram(x, base, width=W, flatten=flatten)
            assert tuple(sp.image.shape) == (B, base.plan.nbands, W) and sp.image.dtype == torch.float32 and sp.image.is_cuda
            assert np.array_equal(bits(sp.image.cpu().numpy()), bits(ref_raster(db, W))), (flatten, W)
            assert sp.duration == n / 44100.0 and sp.columns == [d.shape[-1] for d in db]
            assert np.array_equal(sp.freqs, band_frequencies(base.plan)) and sp.freqs.shape == (base.plan.nbands,)
    assert sp.freqs[0] == 0.0 and abs(sp.freqs[1] - PLANS[pk][2]) < 1e-3 and sp.freqs[-1] == 22050.0


def test_repeatability():
    from xumx_slicq_amd.visualization import spectrogram
    x, _, _ = forward_of("mel", 40000, 1)
    a = spectrogram(x, base_of("mel"), width=64, per_block=True)
    b = spectrogram(x, base_of("mel"), width=64, per_block=True)
    assert np.array_equal(bits(a.image.cpu().numpy()), bits(b.image.cpu().numpy()))
    assert np.array_equal(bits(a.vmax), bits(b.vmax)) and np.array_equal(bits(a.block_vmax), bits(b.block_vmax))
    for u, v in zip(a.blocks, b.blocks):
        assert torch.equal(u, v)


def test_silent_inputs(tmp_path):
    from xumx_slicq_amd.visualization import save_png, spectrogram
    base = base_of("mel")
    sp = spectrogram(noise(5000, 2, "silent").cuda(), base, width=64)
    img = sp.image.cpu().numpy()
    assert np.isneginf(img).all() and np.isneginf(sp.vmax).all() and np.isneginf(sp.vmin).all()
    path = str(tmp_path / "silent.png")
    save_png(path, sp.image[0], sp.vmin[0], sp.vmax[0])
    assert os.path.getsize(path) > 50 and open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    for flatten in (False, True):                              # one silent channel: the mean of anything with -inf is -inf
        for d in device_db("mel", 5000, 2, flatten, "half"):
            assert np.isneginf(d).all()
    sp = spectrogram(noise(5000, 2, "half").cuda(), base, width=7)
    assert np.isneginf(sp.image.cpu().numpy()).all() and np.isneginf(sp.vmax).all()


def test_non_default_stream_gives_the_same_bits():
    from xumx_slicq_amd.visualization import spectrogram
    x, _, _ = forward_of("mel", 5000, 2)
    base = base_of("mel")
    want = spectrogram(x, base, width=64, per_block=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = spectrogram(x, base, width=64, per_block=True)
        img = got.image.cpu().numpy()
    s.synchronize()
    assert np.array_equal(bits(img), bits(want.image.cpu().numpy()))
    assert np.array_equal(bits(got.vmax), bits(want.vmax)) and np.array_equal(bits(got.block_vmax), bits(want.block_vmax))


def test_errors_name_the_problem():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.visualization import overlap_add_slicq, spectrogram
    base = base_of("mel")
    with pytest.raises(ValueError, match="too short"):
        spectrogram(torch.zeros(1, 2, 100, device="cuda"), base)
    with pytest.raises(ValueError, match=r"\(B, 2, n\)"):
        spectrogram(torch.zeros(2, 100, device="cuda"), base)
    with pytest.raises(ValueError, match="T % 4"):
        overlap_add_slicq(torch.zeros(2, 1, 3, 6, dtype=torch.complex64, device="cuda"))
    with pytest.raises(_lib.XsqError):
        spectrogram(torch.zeros(1, 2, 5000), base)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_cli_smoke(tmp_path):
    from xumx_slicq_amd.audio import save_wav_float
    from xumx_slicq_amd.visualization import spectrogram
    n = 2 * 44100
    x = noise(n, 1)
    wav = str(tmp_path / "two seconds.wav")
    save_wav_float(wav, x[0], 44100)
    out = str(tmp_path / "plots")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "xumx_slicq_amd.visualization", "--input-wav", wav, "--out-dir", out, "--width", "64", "--fscale", "mel",
                        "--fbins", "32", "--fmin", "115.5", "--per-block", "--cmap", "gray"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    nblocks = len(base_of("mel").plan.blocks)
    names = sorted(os.listdir(out))
    assert names == sorted(["two seconds.png", "two seconds.json"] + [f"two seconds-block-{i}.png" for i in range(nblocks)])
    for name in names:
        if name.endswith(".png"):
            assert open(os.path.join(out, name), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    info = json.load(open(os.path.join(out, "two seconds.json")))
    sp = spectrogram(x.cuda(), base_of("mel"), width=64, per_block=True)
    assert info["vmax"] == float(sp.vmax[0]) and info["vmin"] == float(sp.vmin[0]) and info["duration"] == 2.0
    assert info["freqs"] == sp.freqs.tolist() and info["block_vmax"] == sp.block_vmax[:, 0].tolist() and info["width"] == 64
