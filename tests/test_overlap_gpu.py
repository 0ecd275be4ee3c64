"""Overlapped, cross-faded segments on the MI355X: xsq_crossfade_place alone against a float64 evaluation of its formula,
Separator.forward_overlapped against its definition (forward per segment, blended in float64), and the CLI.

Bounds, derived: where the weight is 1 the result is the segment's own value, bitwise.  In a fade the result is
fl(fl(w_out * a) + fl(w_in * b)) with w_in = fl(i / (ov - 1)), w_out = fl((ov - 1 - i) / (ov - 1)): one rounding for each
weight, each product and the sum, so |out - exact| <= 4 * 2^-23 * (|w_out * a| + |w_in * b|) with margin."""
import numpy as np
import pytest
import torch

from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
SEGMENT, OVERLAP = 0.25, 0.05
CHUNK_LEN, OV = 11576, 2205
EPS4 = 4 * 2.0 ** -23


def weights64(ov):
    if ov == 1:
        return np.zeros(1), np.ones(1)
    i = np.arange(ov, dtype=np.float64)
    return i / (ov - 1), 1 - i / (ov - 1)


def rule(N, chunk_len, ov):
    start = lambda k: 0 if k == 0 else k * chunk_len - ov
    exists = lambda k: start(k) < N - ov
    out, k = [], 0
    while exists(k):
        out.append((start(k), min((k + 1) * chunk_len, N) - start(k), 0 if k == 0 else ov, ov if exists(k + 1) else 0))
        k += 1
    return out


def blend64(N, segs, ests, ov):
    """(exact float64 blend, sum of |w * v| per sample, mask of the samples inside a fade) of per-segment estimates
    ests[k] (..., n_k) float32 numpy."""
    lead = ests[0].shape[:-1]
    exact, mag, faded = np.zeros(lead + (N,)), np.zeros(lead + (N,)), np.zeros(N, dtype=bool)
    for (start, n, fi, fo), e in zip(segs, ests):
        assert e.shape == lead + (n,) and fi + fo <= n
        w = np.ones(n)
        if fi:
            w[:fi] = weights64(ov)[0]
            faded[start:start + fi] = True
        if fo:
            w[n - fo:] = weights64(ov)[1]
            faded[start + n - fo:start + n] = True
        term = w * e.astype(np.float64)
        exact[..., start:start + n] += term
        mag[..., start:start + n] += np.abs(term)
    return exact, mag, faded


def assert_blend(out, exact, mag, faded, what):
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == exact.shape, what
    plain = exact[..., ~faded].astype(np.float32)
    assert np.array_equal(out[..., ~faded], plain), (what, "outside the fades")
    err = np.abs(out[..., faded].astype(np.float64) - exact[..., faded])
    lim = EPS4 * mag[..., faded]
    worst = float((err - lim).max()) if err.size else 0.0
    print(f"{what}: fade samples {err.size}, max err {float(err.max()) if err.size else 0.0:.3e}, max err / bound "
          f"{float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0:.3f}")
    assert worst <= 0.0, (what, worst)


# ---- the kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("pred", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("ov", [0, 1, 2, 2205])
def test_crossfade_place_against_float64(ov, k, pred, nb):
    """Random scratch rows at odd offsets, an odd start and odd N: k = 3 segments of stride 2311 (odd, >= ov), k = 1 a
    segment that fades out to a successor (no predecessor) or a LAST segment of ov + 1 samples behind a predecessor whose
    stored tail fl(w_out * a) it is added onto.  Samples outside the covered range keep a sentinel."""
    from xumx_slicq_amd import _lib
    rng = np.random.default_rng(1000 * ov + 100 * k + 10 * int(pred) + nb)
    if k == 3:
        stride, n, fade_out = 2311, 2311 + ov, 1
    elif pred:
        stride, n, fade_out = 0, ov + 1, 0
    else:
        stride, n, fade_out = 0, 2 * ov + 37, 1
    start = 1237
    covered = (k - 1) * stride + n
    N = start + covered + 1001
    B = k * nb
    slot = n + 3
    perm = rng.permutation(8 * B)
    rows = perm.astype(np.int64) * slot + 1                          # (target, segment * nb + b, c) -> odd float offsets
    scratch = rng.standard_normal(8 * B * slot + 8).astype(np.float32)
    sentinel = np.float32(-7777.25)
    dst = np.full((4, nb, 2, N), sentinel, dtype=np.float32)
    w_in64, w_out64 = weights64(ov) if ov else (None, None)
    prev = None
    if pred and ov:
        # what the previous pass's launch stored: fl(w_out * a), the weight the fp32 quotient the kernel forms
        prev = rng.standard_normal((4, nb, 2, ov)).astype(np.float32)
        w_out32 = np.ones(1, np.float32) if ov == 1 else (np.arange(ov - 1, -1, -1, dtype=np.float32) / np.float32(ov - 1))
        dst[..., start:start + ov] = w_out32 * prev
    ests = []
    for j in range(k):
        e = np.empty((4, nb, 2, n), dtype=np.float32)
        for t in range(4):
            for b in range(nb):
                for c in range(2):
                    o = rows[(t * B + j * nb + b) * 2 + c]
                    e[t, b, c] = scratch[o:o + n]
        ests.append(e)
    segs = [(start + j * stride, n, ov if (j > 0 or pred) else 0, ov if (j < k - 1 or fade_out) else 0) for j in range(k)]
    exact, mag, faded = blend64(N, segs, ests, ov)
    if prev is not None:
        exact[..., start:start + ov] += w_out64 * prev.astype(np.float64)
        mag[..., start:start + ov] += np.abs(w_out64 * prev.astype(np.float64))
    d_scratch, d_rows, d_dst = torch.from_numpy(scratch).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(dst).cuda()
    _lib.check(_lib.lib.xsq_crossfade_place(d_scratch.data_ptr(), d_rows.data_ptr(), d_dst.data_ptr(), nb, N, start, stride, n, k, ov,
                                            1 if pred else 0, fade_out, _lib.stream_ptr()), "xsq_crossfade_place")
    got = d_dst.cpu().numpy()
    assert np.all(got[..., :start] == sentinel) and np.all(got[..., start + covered:] == sentinel)
    assert torch.equal(d_scratch.cpu(), torch.from_numpy(scratch))
    assert_blend(got[..., start:start + covered], exact[..., start:start + covered], mag[..., start:start + covered],
                 faded[start:start + covered], f"kernel ov={ov} k={k} pred={pred} nb={nb}")


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seps():
    from xumx_slicq_amd.separator import seeded_separator
    return {"mixphase": seeded_separator(realtime=True), "niter1": seeded_separator(realtime=False, niter=1),
            "niter2": seeded_separator(realtime=False, niter=2)}


@pytest.fixture(scope="module")
def track():
    x = synth_audio(60000, seed=4711, nb_samples=2)
    x[1] *= 3.0
    return x.cuda()


@pytest.fixture(scope="module")
def segment_stems(seps, track):
    """forward(segment) per (separator, nb, start, n), computed once: segments of different N share all but the last."""
    cache = {}

    def get(name, nb, start, n):
        key = (name, nb, start, n)
        if key not in cache:
            cache[key] = seps[name](track[:nb, :, start:start + n]).cpu().numpy()
        return cache[key]
    return get


def reference(segment_stems, name, nb, N, chunk_len=CHUNK_LEN, ov=OV):
    segs = rule(N, chunk_len, ov)
    return segs, blend64(N, segs, [segment_stems(name, nb, s, n) for s, n, _, _ in segs], ov)


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("N", [11576, 11577, 23152, 23153, 60000])
@pytest.mark.parametrize("name", ["mixphase", "niter1", "niter2"])
def test_forward_overlapped_is_the_blend_of_forward_per_segment(seps, track, segment_stems, name, N, nb):
    """N: one segment; a last segment of ov + 1; a segment end on N exactly; three segments with a minimal last one; six
    segments.  Outside the fades bitwise forward(segment) -- for N = 11576 the whole track, its last ov samples too (a
    segment without a successor does not fade out) -- and inside them within the derived bound."""
    from xumx_slicq_amd.separator import segment_lengths, segments
    sep = seps[name]
    assert segment_lengths(float(sep.sample_rate), SEGMENT, OVERLAP, sep.chunk_size) == (CHUNK_LEN, OV)
    segs, (exact, mag, faded) = reference(segment_stems, name, nb, N)
    assert segments(N, CHUNK_LEN, OV) == segs
    assert len(segs) == {11576: 1, 11577: 2, 23152: 2, 23153: 3, 60000: 6}[N]
    if N in (11577, 23153):
        assert segs[-1][1] == OV + 1
    x = track[:nb, :, :N].contiguous()
    x0 = x.clone()
    out = sep.forward_overlapped(x, SEGMENT, OVERLAP)
    assert out.shape == (4, nb, 2, N) and out.dtype == torch.float32 and torch.equal(x, x0)
    if N == 11576:
        assert not faded.any() and torch.equal(out, sep(x))
    assert_blend(out.cpu().numpy(), exact, mag, faded, f"{name} N={N} nb={nb}")


@pytest.mark.parametrize("name", ["mixphase", "niter1"])
def test_pass_grouping_does_not_show(seps, track, name):
    """Six segments, the four middle ones in one pass (max_stack = 8 against a chunk_size of one segment: 8 items of 3
    slices), in two passes (max_stack = 2) and one per pass (max_item_slices = 3): the heads a pass adds onto the tail
    the previous launch stored are the bits a single launch forms.  The default chunk_size, where all four stack whatever
    max_stack says, and a second call agree too."""
    sep = seps[name]
    x = track[:1, :, :60000].contiguous()
    base = sep.forward_overlapped(x, SEGMENT, OVERLAP)
    assert torch.equal(base, sep.forward_overlapped(x, SEGMENT, OVERLAP))
    try:
        sep.chunk_size = CHUNK_LEN + OV
        sizes = []
        for max_stack, cap in ((8, 0), (2, 0), (8, 3)):
            sep.max_stack, sep.max_item_slices = max_stack, cap
            assert torch.equal(base, sep.forward_overlapped(x, SEGMENT, OVERLAP)), (max_stack, cap)
            sizes += [v for k, v in sep._nsizes.items() if k[0] == "segments" and k[3] == CHUNK_LEN + OV and k[6] == max_stack and k[-1] == cap]
        assert len(sizes) == 3 and sizes[0] > sizes[1] > sizes[2], sizes        # 4, 2 and 1 middle segments per pass: smaller workspaces
    finally:
        sep.chunk_size, sep.max_stack, sep.max_item_slices = 2621440, 8, 0
    x2 = track[:, :, :60000].contiguous()
    base2 = sep.forward_overlapped(x2, SEGMENT, OVERLAP)
    try:
        sep.max_item_slices = 6                      # nb = 2: one (segment, batch) item of 2 * 3 slices per pass
        assert torch.equal(base2, sep.forward_overlapped(x2, SEGMENT, OVERLAP))
    finally:
        sep.max_item_slices = 0


@pytest.mark.parametrize("name", ["mixphase", "niter1"])
def test_overlap_zero_is_forward_with_chunk_size_chunk_len(seps, track, name):
    sep = seps[name]
    x = track[:, :, :60000 - 3].contiguous()
    got = sep.forward_overlapped(x, SEGMENT, 0.0)
    try:
        sep.chunk_size = 11025
        want = sep(x)
    finally:
        sep.chunk_size = 2621440
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["mixphase", "niter2"])
def test_python_fallback_meets_the_same_bound(seps, track, segment_stems, name):
    sep = seps[name]
    N, nb = 23153, 2
    _, (exact, mag, faded) = reference(segment_stems, name, nb, N)
    x = track[:nb, :, :N].contiguous()
    try:
        sep.native = False
        out = sep.forward_overlapped(x, SEGMENT, OVERLAP)
    finally:
        sep.native = True
    assert_blend(out.cpu().numpy(), exact, mag, faded, f"fallback {name}")


def test_cli_segment_overlap_writes_forward_overlapped(tmp_path, seps):
    import subprocess
    import sys

    from conftest import ROOT
    from xumx_slicq_amd import audio as A
    (tmp_path / "in").mkdir()
    A.save_wav_float(str(tmp_path / "in" / "clip.wav"), synth_audio(44100, seed=96)[0], 44100)
    subprocess.run([sys.executable, "-m", "xumx_slicq_amd", "--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out"),
                    "--segment", str(SEGMENT), "--overlap", str(OVERLAP)], check=True, cwd=ROOT, timeout=300)
    sep = seps["niter1"]                                  # the CLI's default model: the offline stack, one EM iteration
    x, rate = A.load_audio(str(tmp_path / "in" / "clip.wav"))
    want = sep.forward_overlapped(x[None].cuda(), SEGMENT, OVERLAP).cpu()
    assert sorted(p.name for p in (tmp_path / "out" / "clip").iterdir()) == sorted(f"{t}.wav" for t in sep.sources)
    for t, target in enumerate(sep.sources):
        y, rate = A.load_audio(str(tmp_path / "out" / "clip" / f"{target}.wav"))
        assert rate == 44100 and torch.equal(y, want[t, 0]), target
