"""Overlapped, cross-faded segments without a GPU: the segment rule of xsq_segment_schedule against a restatement of it,
its invariants, the refusals of the C entry points and of the Python front, the CLI options and the input-shape rules of
cadenza.separate_sources on a stub model."""
import ctypes as C

import numpy as np
import pytest
import torch

SR = 44100
PAIRS = ((0.25, 0.05), (0.25, 0.1), (0.3, 0.2), (10.0, 0.1), (0.21, 0.5))


def lengths(segment, overlap, sr=SR):
    return int(sr * segment * (1 + overlap)), int(overlap * sr)


def rule(N, chunk_len, ov):
    """The segment rule, restated: (start, samples, fade_in, fade_out) per segment."""
    start = lambda k: 0 if k == 0 else k * chunk_len - ov
    exists = lambda k: start(k) < N - ov
    out, k = [], 0
    while exists(k):
        out.append((start(k), min((k + 1) * chunk_len, N) - start(k), 0 if k == 0 else ov, ov if exists(k + 1) else 0))
        k += 1
    return out


def schedule(N, chunk_len, ov):
    from xumx_slicq_amd import _lib
    buf = np.zeros((64, 4), dtype=np.int64)
    n = _lib.lib.xsq_segment_schedule(N, chunk_len, ov, buf.ctypes.data, len(buf))
    assert 0 <= n <= len(buf), (n, _lib.last_error())
    return [tuple(r) for r in buf[:n].tolist()]


def grid():
    """(segment, overlap, N): N within +-3 of k * chunk_len and k * chunk_len +- ov, k = 1..4 (N >= 1)."""
    cases = []
    for segment, overlap in PAIRS:
        chunk_len, ov = lengths(segment, overlap)
        Ns = {c + d for k in range(1, 5) for c in (k * chunk_len, k * chunk_len - ov, k * chunk_len + ov) for d in range(-3, 4)}
        cases += [(segment, overlap, N) for N in sorted(Ns) if N >= 1]
    return cases


def test_segment_schedule_is_the_rule_on_the_grid():
    cases = grid()
    assert len(cases) == 413
    for segment, overlap, N in cases:
        chunk_len, ov = lengths(segment, overlap)
        assert schedule(N, chunk_len, ov) == rule(N, chunk_len, ov), (segment, overlap, N)
    # the defaults on the 240 s bench track
    s = schedule(10_584_000, *lengths(10.0, 0.1))
    assert len(s) == 22 and s[0][:2] == (0, 485100) and s[-1][:2] == (10182690, 401310)
    assert all(q[1] == 489510 for q in s[1:-1])
    assert abs(sum(q[1] for q in s) / 10_584_000 - 1.009) < 5e-4


def test_segment_invariants_on_the_grid():
    """Consecutive segments share exactly ov samples, the segments cover [0, N), the last one has more than ov samples and
    what one segment fades out the next fades in.  Held wherever the rule describes a cover at all, ov < chunk_len and
    N > ov -- what the separator accepts.  The pair (0.21, 0.5) has ov = 22050 > chunk_len = 13891 (its second segment would
    start at a negative sample), and the seven N around chunk_len - ov = 7056 of (0.3, 0.2) are below ov = 8820, where the
    rule has no segment at all (`start_0 < N - ov` fails): those are held against the restated rule only, above."""
    held = skipped = 0
    for segment, overlap, N in grid():
        chunk_len, ov = lengths(segment, overlap)
        if ov >= chunk_len or N <= ov:
            assert (segment, overlap) == (0.21, 0.5) or ((segment, overlap) == (0.3, 0.2) and schedule(N, chunk_len, ov) == [])
            skipped += 1
            continue
        s = schedule(N, chunk_len, ov)
        assert s and s[0][0] == 0 and s[0][2] == 0 and s[-1][3] == 0
        assert s[-1][0] + s[-1][1] == N and s[-1][1] > ov
        for a, b in zip(s, s[1:]):
            assert a[0] + a[1] - b[0] == ov and b[0] > a[0]
            assert a[3] == b[2] == ov
        for a, c in zip(s, s[2:]):
            assert a[0] + a[1] <= c[0]
        held += 1
    assert held + skipped == 413 and skipped == sum(1 for q in grid() if q[:2] == (0.21, 0.5)) + 7


def test_c_entry_points_refuse_bad_arguments():
    from xumx_slicq_amd import _lib
    L = _lib.lib
    buf = np.zeros((8, 4), dtype=np.int64)
    for N, cl, ov, word in ((0, 10, 1, "N=0"), (100, 0, 0, "chunk_len=0"), (100, 10, -1, "ov=-1")):
        assert L.xsq_segment_schedule(N, cl, ov, buf.ctypes.data, 8) < 0 and word in _lib.last_error()
    assert L.xsq_segment_schedule(100, 10, 1, None, 8) < 0
    assert L.xsq_segment_schedule(5, 10, 5, buf.ctypes.data, 8) == 0            # N <= ov: no segment exists
    assert L.xsq_segment_schedule(1000, 10, 1, None, 0) == 100                  # count only
    dummy = C.create_string_buffer(4096)
    h = C.addressof(dummy)

    def fwd(cs, cl, ov, N=100000, nb=1, d=h, audio=h):
        return L.xsq_separator_forward_segments(d, h, audio, nb, N, cs, cl, ov, 8, 0, h, h, 4096, None)

    def wsp(cs, cl, ov, N=100000):
        b = C.c_size_t()
        return L.xsq_separator_segments_workspace(h, h, 1, N, cs, cl, ov, 8, 0, C.byref(b))

    for call in (fwd, wsp):
        for args, word in (((20000, 11576, 9000), "longer than chunk_size"), ((20000, 30000, 0), "longer than chunk_size"),
                           ((20000, 1000, 1000), ">= chunk_len"), ((20000, 1000, 1500), ">= chunk_len"),
                           ((20000, 1000, -1), "ov=-1"), ((20000, 0, 0), "chunk_len=0"), ((20000, -5, 0), "chunk_len=-5")):
            assert call(*args) < 0, args
            assert word in _lib.last_error(), (args, _lib.last_error())
        assert call(20000, 11576, 2205, N=2205) < 0 and "no segment" in _lib.last_error()
    assert fwd(20000, 11576, 2205, d=None) < 0 and "null" in _lib.last_error()
    assert fwd(20000, 11576, 2205, audio=None) < 0 and "null" in _lib.last_error()
    assert fwd(20000, 11576, 2205, nb=0) < 0

    def place(scratch=h, nb=1, N=1000, start=0, stride=90, n=100, k=2, ov=10, fi=0, fo=0):
        return L.xsq_crossfade_place(scratch, h, h, nb, N, start, stride, n, k, ov, fi, fo, None)

    assert place(scratch=None) < 0 and "null" in _lib.last_error()
    for kw in (dict(nb=0), dict(n=0), dict(k=0), dict(ov=-1), dict(start=-1), dict(stride=80), dict(stride=95, n=100, ov=5, k=2, N=150),
               dict(stride=40, n=100, ov=60), dict(k=1, ov=60, fi=1, fo=1), dict(k=1, n=100, ov=101), dict(N=150)):
        assert place(**kw) < 0, kw


def test_forward_overlapped_refuses_bad_arguments():
    from xumx_slicq_amd.separator import Separator, segment_lengths
    assert segment_lengths(44100.0, 10.0, 0.1) == (485100, 4410)
    assert segment_lengths(44100, 0.25, 0.05) == (11576, 2205)
    assert segment_lengths(44100, 0.25, 0.0, chunk_size=11025) == (11025, 0)
    for segment, overlap in ((0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (10.0, -0.01), (10.0, 1.0), (10.0, 1.5),
                             (10.0, float("nan")), (0.21, 0.5), (1e-6, 0.0)):
        with pytest.raises(ValueError):
            segment_lengths(44100, segment, overlap)
    with pytest.raises(ValueError, match="chunk_size"):
        segment_lengths(44100, 10.0, 0.1, chunk_size=485100 + 4409)
    assert segment_lengths(44100, 10.0, 0.1, chunk_size=485100 + 4410) == (485100, 4410)

    class Stub(Separator):                    # the argument checks come before any device work
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.register_buffer("sample_rate", torch.as_tensor(44100.0))
            self.chunk_size = 20000

    sep = Stub()
    x = torch.zeros(1, 2, 30000)
    for segment, overlap in ((0.0, 0.1), (0.25, 1.0), (0.25, -0.1), (1.0, 0.1)):      # (1.0, 0.1): longer than chunk_size
        with pytest.raises(ValueError):
            sep.forward_overlapped(x, segment, overlap)
    with pytest.raises(ValueError, match="no segment"):
        sep.forward_overlapped(torch.zeros(1, 2, 2205), 0.25, 0.05)
    with pytest.raises(ValueError):
        sep.forward_overlapped(torch.zeros(2, 30000), 0.25, 0.05)


def test_cli_segment_overlap_and_remix_options(capsys):
    from xumx_slicq_amd.inference import cli_parser, inference_main, overlapped_option, parse_args
    p = cli_parser()
    assert overlapped_option(parse_args(p, [])) is None
    assert overlapped_option(parse_args(p, ["--segment", "5"])) == (5.0, 0.1)
    assert overlapped_option(parse_args(p, ["--overlap", "0.25"])) == (10.0, 0.25)
    assert overlapped_option(parse_args(p, ["--segment", "0.25", "--overlap", "0"])) == (0.25, 0.0)
    for argv, word in ((["--segment", "5", "--remix", "karaoke:vocals=0"], "not built"),
                       (["--overlap", "0.1", "--remix", "karaoke:vocals=0"], "not built"),
                       (["--segment", "0"], "--segment"), (["--segment", "-2"], "--segment"), (["--segment", "nan"], "--segment"),
                       (["--overlap", "1"], "--overlap"), (["--overlap", "-0.1"], "--overlap"), (["--overlap", "nan"], "--overlap")):
        with pytest.raises(SystemExit) as e:
            inference_main(argv + ["--device", "cpu"])
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


class _StubModel(torch.nn.Module):
    """forward (nb, ch, n) -> (4, nb, ch, n): target t is (t + 1) * the input -- linear and memoryless, so the faded sum of
    the segments gives the same back wherever the weights sum to 1."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        return torch.stack([(t + 1) * x for t in range(4)])


def test_separate_sources_input_shapes_on_a_stub_model():
    from xumx_slicq_amd.cadenza import separate_sources
    rng = np.random.default_rng(5)
    sr, segment, overlap = 8000, 0.25, 0.05
    chunk_len, ov = lengths(segment, overlap, sr)                 # 2100, 400
    for shape in ((9000,), (2, 9000), (3, 2, 9000), (1, 1, chunk_len)):
        mix = rng.standard_normal(shape).astype(np.float32)
        for arg in (mix, torch.from_numpy(mix)):
            m = _StubModel()
            out = separate_sources(m, arg, sr, segment=segment, overlap=overlap)
            want3 = mix[None] if mix.ndim == 2 else mix[None, None] if mix.ndim == 1 else mix
            assert isinstance(out, np.ndarray) and out.shape == (want3.shape[0], 4) + want3.shape[1:]
            assert [c[-1] for c in m.calls] == [q[1] for q in rule(shape[-1], chunk_len, ov)]
            for t in range(4):
                np.testing.assert_allclose(out[:, t], (t + 1) * want3, rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        separate_sources(_StubModel(), np.zeros((1, 1, 2, 100), np.float32), sr)
    with pytest.raises(ValueError):
        separate_sources(_StubModel(), np.zeros(9000, np.float32), sr, segment=0.25, overlap=1.0)
    # a single short segment is not faded out (the documented departure from the reference)
    m = _StubModel()
    mix = rng.standard_normal((2, 1000)).astype(np.float32)
    out = separate_sources(m, mix, sr, segment=segment, overlap=overlap)
    assert np.array_equal(out[0, 0], mix) and m.calls == [(1, 2, 1000)]
