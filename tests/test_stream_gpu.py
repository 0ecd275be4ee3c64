"""``Separator.stream`` on the MI355X: a session fed block by block returns ``forward`` of the whole signal.

The bound of the comparisons is not a constant: with e_fwd the error of ``forward(whole)`` and e_str the error of the joined
session, both against ``oracle.ref64.separate`` in float64 on the same input by ``ref64.rel_err`` (RMS and max), the tests require
e_str <= 2 * e_fwd for both.  The two are fp32 evaluations of the same sums under possibly different tilings (the window of a step
starts at another slice parity than the whole call's arena, which moves individual roundings of the F(2, 2) / Winograd kernels, not
their scale); a window one slice short sits near 1e-3 RMS, four orders above (tests/test_stream_cpu.py).  Every case prints both
figures; DESIGN.md 4.11 holds the measured ones.

Sections 9 to 11 hold the fused L = 18060 kernels of Bark-262 where a step inverts several new slices onto a carried half (m >= 2),
the offline stack, two items and the short signals, long Mel-32 sessions, and what the header promises of the state and the
workspace; the two transform halves of a step are judged per band and per block in tests/test_stream_stages_gpu.py.
"""
import numpy as np
import pytest
import torch

from oracle import ref64
from test_ref64_mel_cpu import MEL, SEED, make_mel_plan, make_mel_sd
from test_streams_gpu import run_delayed

pytestmark = pytest.mark.gpu

L = 2016
H = L // 4
N_TRACK = 23 * H + 17
FEED = 700
MODELS = {"realtime": True, "offline_phasemix": False}          # name -> causal


@pytest.fixture(scope="module")
def mel_seps():
    from xumx_slicq_amd.separator import seeded_separator
    cfg = dict(fscale=MEL[0], fbins=MEL[1], fmin=MEL[2], seed=SEED)
    return {"realtime": seeded_separator(realtime=True, **cfg), "offline_phasemix": seeded_separator(realtime=False, wiener=False, **cfg)}


@pytest.fixture(scope="module")
def mel_tables():
    plan = make_mel_plan()
    return plan, make_mel_sd(plan)


@pytest.fixture(scope="module")
def mel_ref(mel_tables):
    """float64 stems of (model, nb, N), computed once and shared by the cases that differ in hop_slices or in the arm."""
    plan, sd = mel_tables
    cache = {}

    def get(name, nb, n):
        key = (name, nb, n)
        if key not in cache:
            cache[key] = ref64.separate(plan, sd, track(nb, n), causal=MODELS[name], wiener=False)
        return cache[key]
    return get


def track(nb, n):
    return 2 * torch.rand(nb, 2, n, generator=torch.Generator().manual_seed(1000 * nb + n)) - 1


def run_session(sep, x, hop_slices=1, feeds=FEED, prepare=None):
    """The joined returns of a session over ``x``, fed in blocks of ``feeds`` samples (an int) or of the listed sizes; ``prepare`` is
    called with the session before its first feed."""
    n = x.shape[-1]
    sizes = [min(feeds, n - p) for p in range(0, n, feeds)] if isinstance(feeds, int) else list(feeds)
    assert sum(sizes) == n
    session = sep.stream(x.shape[0], hop_slices)
    assert session._native == sep._native_switches()
    if prepare is not None:
        prepare(session)
    per, parts, p = 2 * session.h * hop_slices, [], 0
    for k in sizes:
        parts.append(session.feed(x[..., p:p + k]))
        p += k
        assert parts[-1].shape[:3] == (4, x.shape[0], 2) and parts[-1].shape[-1] % per == 0
        assert session.samples_in == p and session.samples_out == sum(q.shape[-1] for q in parts)
    parts.append(session.flush())
    assert session.samples_out == n
    return torch.cat(parts, dim=-1)


def judge(what, est_stream, est_forward, ref):
    e_fwd, e_str = ref64.rel_err(est_forward, ref), ref64.rel_err(est_stream, ref)
    bitwise = torch.equal(est_stream, est_forward)
    print(f"[stream] {what}: e_fwd rms {float(e_fwd[0]):.3e} max {float(e_fwd[1]):.3e} | e_str rms {float(e_str[0]):.3e} max {float(e_str[1]):.3e}"
          f" | stream vs forward max abs {float((est_stream - est_forward).abs().max()):.3e}{' (bitwise equal)' if bitwise else ''}")
    assert est_stream.shape == est_forward.shape == ref.shape
    assert float(e_str[0]) <= 2 * float(e_fwd[0]) and float(e_str[1]) <= 2 * float(e_fwd[1]), what


# ---- 1. Mel-32, both mix-phase stacks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop_slices", [1, 2])
@pytest.mark.parametrize("n", [1, 1009, 2 * H, N_TRACK])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_mel_session_is_forward_of_the_whole(mel_seps, mel_ref, name, nb, n, hop_slices):
    sep = mel_seps[name]
    x = track(nb, n).cuda()
    judge(f"{name} nb={nb} n={n} m={hop_slices}", run_session(sep, x, hop_slices).cpu(), sep.forward(x).cpu(), mel_ref(name, nb, n))


def test_mel_session_where_forward_takes_its_long_row_kernels(mel_seps, mel_ref):
    """From 65 slices on the whole call's CDAE runs other kernels than a window of m + 5 slices does (rows of S * T positions select
    them), so the two are no longer the same bits -- every shorter case of this module is -- and the bound has something to hold:
    measured 2.7e-7 max between the two, at a signal RMS of 0.17."""
    sep = mel_seps["realtime"]
    n = 2 * H * 64 + 17
    x = track(1, n).cuda()
    judge(f"realtime nb=1 n={n} m=8", run_session(sep, x, 8, 4096).cpu(), sep.forward(x).cpu(), mel_ref("realtime", 1, n))


# ---- 2. Bark-262: the only plan with frequency taps (kf = 3 and 5) ---------------------------------------------------------
def test_bark_realtime_session_is_forward_of_the_whole(oracle_plan, seeded_sd):
    from xumx_slicq_amd.separator import seeded_separator
    sep = seeded_separator(realtime=True)
    n = 100000
    assert oracle_plan.nslices(n) == 13
    x = track(1, n)
    ref = ref64.separate(oracle_plan, seeded_sd, x, causal=True, wiener=False)
    xd = x.cuda()
    judge(f"bark realtime n={n} m=1", run_session(sep, xd, 1, 30000).cpu(), sep.forward(xd).cpu(), ref)


# ---- 3. the result does not depend on the partition into feeds -------------------------------------------------------------
@pytest.mark.parametrize("hop_slices", [1, 2])
def test_partition_of_the_feeds_does_not_change_a_bit(mel_seps, hop_slices):
    sep = mel_seps["realtime"]
    x = track(1, N_TRACK).cuda()
    n = N_TRACK
    want = run_session(sep, x, hop_slices, [n])
    for feeds in ([1, n - 1], FEED, 2 * H, [5000, 0, 0, n - 5000], [n - 1, 1]):
        got = run_session(sep, x, hop_slices, feeds)
        assert torch.equal(got, want), (feeds, float((got - want).abs().max()))


# ---- 4. latency and bookkeeping -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop_slices", [1, 3])
def test_steps_fire_on_the_grid_and_flush_closes_the_session(mel_seps, hop_slices):
    from xumx_slicq_amd._lib import XsqError
    sep, m = mel_seps["realtime"], hop_slices
    assert sep.stream(1, m).latency_samples == 8 * H
    for j in (0, 2):
        need = (2 * (j + 1) * m + 6) * H
        x = track(1, need + 5).cuda()
        for fed, steps in ((need, j + 1), (need - 1, j)):
            s = sep.stream(1, m)
            out = s.feed(x[..., :fed])
            assert s.samples_in == fed and s.samples_out == out.shape[-1] == 2 * H * m * steps, (j, fed)
            more = s.feed(x[..., fed:fed + 1])                     # one more sample releases the step that was one short
            assert more.shape == (4, 1, 2, 2 * H * m * (j + 1 - steps))
            rest = s.flush()
            assert s.samples_out == s.samples_in == fed + 1 == out.shape[-1] + more.shape[-1] + rest.shape[-1]
            with pytest.raises(XsqError):
                s.feed(x[..., :10])
            with pytest.raises(XsqError):
                s.flush()
    s = sep.stream(2, m)
    assert s.feed(torch.zeros(2, 2, 0, device="cuda")).shape == (4, 2, 2, 0)
    assert s.flush().shape == (4, 2, 2, 0) and s.samples_out == 0
    with pytest.raises(ValueError):
        sep.stream(1, m).feed(torch.zeros(2, 2, 10, device="cuda"))


# ---- 5. the state does not grow ---------------------------------------------------------------------------------------------
def test_state_is_bounded_over_400_blocks(mel_seps, mel_tables):
    """... and the last block the session emits, block 399 of the stream, is still ``forward`` of the signal around it: against
    float64 on the 13 blocks 390 .. 402 (the slices 396 .. 402 its masks read lie inside them, clear of the cut ends), under the
    bound of ``judge``."""
    sep = mel_seps["realtime"]
    x = track(1, 2 * H * 40).cuda()
    s = sep.stream(1, 1)
    state, allocated = s.state_bytes, {}
    assert state == s._state.numel() and state >= 4 * (2 * (2 * (3 + 2 + 1) + 2) * H + 2 * 8 * 2 * H)
    last = None
    for k in range(1, 404):
        out = s.feed(x[..., (k % 40) * 2 * H:(k % 40 + 1) * 2 * H])
        assert out.shape[-1] == (2 * H if k >= 4 else 0)
        if k == 403:
            last = out.cpu()                                      # block k - 4 = 399 of the stream (host memory)
        del out
        if k in (23, 403):                                        # after step 20 and after step 400
            assert s.samples_out == 2 * H * (k - 3)
            allocated[k] = torch.cuda.memory_allocated()
        assert s.state_bytes == state
    assert allocated[403] == allocated[23], allocated
    plan, sd = mel_tables
    around = torch.cat([x[..., (k % 40) * 2 * H:(k % 40 + 1) * 2 * H] for k in range(391, 404)], dim=-1)      # fed as blocks 390 .. 402
    cut = slice(9 * 2 * H, 10 * 2 * H)
    ref = ref64.separate(plan, sd, around.cpu(), causal=True, wiener=False)[..., cut]
    judge("realtime block 399 of a 403-block session", last, sep.forward(around).cpu()[..., cut], ref)


# ---- 6. the stream contract -------------------------------------------------------------------------------------------------
def test_session_on_a_side_stream_behind_a_delayed_producer(mel_seps):
    sep = mel_seps["realtime"]
    x, decoy = track(1, N_TRACK).cuda(), 3 * track(1, N_TRACK + 1)[..., 1:].cuda()
    want = run_delayed("stream session", lambda a: run_session(sep, a), x, decoy, owners=(sep,))
    assert torch.equal(want[0], run_session(sep, x))


def test_two_sessions_on_two_streams_interleaved(mel_seps):
    sep = mel_seps["realtime"]
    xs = [track(1, N_TRACK).cuda(), track(1, N_TRACK + 3)[..., 3:].cuda()]
    want = [run_session(sep, x) for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    sessions, parts = [sep.stream(1, 1) for _ in xs], [[], []]
    for p in range(0, N_TRACK, FEED):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                parts[i].append(sessions[i].feed(xs[i][..., p:p + FEED]))
    for i in (0, 1):
        with torch.cuda.stream(streams[i]):
            parts[i].append(sessions[i].flush())
            got = torch.cat(parts[i], dim=-1)
        streams[i].synchronize()
        assert torch.equal(got, want[i]), i
    assert not torch.equal(want[0], want[1])


# ---- 7. the Python arm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_python_arm_meets_the_same_bound(mel_seps, mel_ref, name):
    sep = mel_seps[name]
    x = track(1, N_TRACK).cuda()
    fwd = sep.forward(x).cpu()
    try:
        sep.native = False
        session = sep.stream(1, 2)
        assert not session._native
        est = run_session(sep, x, 2).cpu()
    finally:
        del sep.native
    judge(f"{name} native=False m=2", est, fwd, mel_ref(name, 1, N_TRACK))


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_stream_writes_the_stems_of_the_session(mel_seps, tmp_path, monkeypatch):
    from xumx_slicq_amd import audio as xaudio
    from xumx_slicq_amd import inference
    sep = mel_seps["realtime"]
    x = track(1, N_TRACK)
    (tmp_path / "in").mkdir()
    xaudio.save_wav_float(str(tmp_path / "in" / "clip.wav"), x[0], 44100)
    monkeypatch.setattr(inference, "seeded_separator", lambda **kw: sep)
    inference.inference_main(["--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out"), "--realtime", "--stream", "4096",
                              "--hop-slices", "2"])
    want = run_session(sep, x.cuda(), 2, 4096).cpu()
    for t, target in enumerate(sep.sources):
        got, rate = xaudio.load_audio(str(tmp_path / "out" / "clip" / f"{target}.wav"))
        assert rate == 44100 and torch.equal(got, want[t, 0]), target
    assert np.isfinite(want.numpy()).all()


# ---- 9. Bark-262, the fused L = 18060 slice kernels: several new slices per step, the offline stack, nb = 2 -----------------
BARK_L = 18060
BARK_H = BARK_L // 4
BARK_N = 100000                 # 13 slices, 12 blocks, the last one 670 samples
BARK_FEED = 30000


@pytest.fixture(scope="module")
def bark_seps():
    from xumx_slicq_amd.separator import seeded_separator
    return {"realtime": seeded_separator(realtime=True), "offline_phasemix": seeded_separator(realtime=False, wiener=False)}


@pytest.fixture(scope="module")
def bark_ref(oracle_plan, seeded_sd, bark_seps):
    """(float64 stems, ``forward`` of the whole signal) of (model, nb, N) on ``track(nb, N)``, computed once per module."""
    cache = {}

    def get(name, nb, n):
        key = (name, nb, n)
        if key not in cache:
            x = track(nb, n)
            cache[key] = (ref64.separate(oracle_plan, seeded_sd, x, causal=MODELS[name], wiener=False), bark_seps[name].forward(x.cuda()).cpu())
        return cache[key]
    return get


def bark_case(bark_seps, bark_ref, name, nb, n, hop_slices, feeds=BARK_FEED):
    ref, fwd = bark_ref(name, nb, n)
    judge(f"bark {name} nb={nb} n={n} m={hop_slices}", run_session(bark_seps[name], track(nb, n).cuda(), hop_slices, feeds).cpu(), fwd, ref)


@pytest.mark.parametrize("hop_slices,steps", [(2, 6), (3, 4), (5, 3)])
def test_bark_realtime_session_with_several_new_slices_per_step(oracle_plan, bark_seps, bark_ref, hop_slices, steps):
    """Every step after the first inverts m >= 2 new slices onto the carried half: both launches of the fused inverse kernel run
    beside a carry.  m = 2: the third feed of 30000 samples releases two steps at once and flush runs two clipped ones; m = 5:
    one step in feed, two in flush, the last of 2 blocks cut at n."""
    from xumx_slicq_amd.separator import stream_steps, stream_trigger
    assert oracle_plan.nslices(BARK_N) == 13 and len(stream_steps(BARK_N, BARK_L, hop_slices, 3)) == steps
    assert [stream_trigger(j, BARK_L, 2) for j in range(4)] == [45150, 63210, 81270, 99330]
    bark_case(bark_seps, bark_ref, "realtime", 1, BARK_N, hop_slices)


@pytest.mark.parametrize("hop_slices", [1, 3])
def test_bark_offline_session_is_forward_of_the_whole(bark_seps, bark_ref, hop_slices):
    bark_case(bark_seps, bark_ref, "offline_phasemix", 1, BARK_N, hop_slices)


@pytest.mark.parametrize("hop_slices", [1, 2])
def test_bark_session_of_two_items(bark_seps, bark_ref, hop_slices):
    bark_case(bark_seps, bark_ref, "realtime", 2, 50000, hop_slices)


@pytest.mark.parametrize("hop_slices", [1, 4])
@pytest.mark.parametrize("n", [1, 9031, 18060, 18061])
@pytest.mark.parametrize("name", list(MODELS))
def test_bark_short_signals(bark_seps, bark_ref, name, n, hop_slices):
    bark_case(bark_seps, bark_ref, name, 1, n, hop_slices)


def test_bark_partition_of_the_feeds_does_not_change_a_bit(bark_seps):
    sep, n = bark_seps["realtime"], BARK_N
    x = track(1, n).cuda()
    want = run_session(sep, x, 3, [n])
    for feeds in ([1, n - 1], 9030, BARK_FEED, [50000, 0, n - 50000]):
        got = run_session(sep, x, 3, feeds)
        assert torch.equal(got, want), (feeds, float((got - want).abs().max()))
    assert np.isfinite(want.cpu().numpy()).all()


def test_bark_python_arm_meets_the_same_bound(bark_seps, bark_ref):
    sep = bark_seps["realtime"]
    ref, fwd = bark_ref("realtime", 1, BARK_N)
    try:
        sep.native = False
        assert not sep.stream(1, 3)._native
        est = run_session(sep, track(1, BARK_N).cuda(), 3, BARK_FEED).cpu()
    finally:
        del sep.native
    judge("bark realtime native=False m=3", est, fwd, ref)


# ---- 10. long Mel-32 sessions against float64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("hop_slices", [1, 7])
def test_mel_long_session_is_forward_of_the_whole(mel_seps, mel_ref, hop_slices):
    """n = 300000: 298 blocks; at m = 1 a step per block, and the ring of 14h = 7056 samples turns over 42 times."""
    sep, n = mel_seps["realtime"], 300000
    assert sep.stream(1, 1)._state is not None and (2 * (3 + 2 + 1) + 2) * H == 7056
    x = track(1, n).cuda()
    judge(f"realtime nb=1 n={n} m={hop_slices}", run_session(sep, x, hop_slices, 4096).cpu(), sep.forward(x).cpu(), mel_ref("realtime", 1, n))


# ---- 11. the state needs no initialisation; nothing lives in the workspace between steps --------------------------------------
@pytest.mark.parametrize("which", ["mel", "bark"])
def test_state_needs_no_initialisation(mel_seps, bark_seps, which):
    """The ring and both carry buffers filled with NaN, and with 1e30, before the first feed: the bits of an untouched session."""
    sep, n, feeds = (mel_seps["realtime"], N_TRACK, FEED) if which == "mel" else (bark_seps["realtime"], BARK_N, BARK_FEED)
    x = track(1, n).cuda()
    want = run_session(sep, x, 2, feeds)
    assert np.isfinite(want.cpu().numpy()).all()
    for fill in (float("nan"), 1e30):
        def prepare(session):
            state = session._state.view(torch.float32)
            assert state.numel() * 4 == session.state_bytes
            state.fill_(fill)
        got = run_session(sep, x, 2, feeds, prepare=prepare)
        assert torch.equal(got, want), (which, fill)


def test_two_sessions_and_a_forward_share_one_stream(mel_seps):
    """Two sessions of different hop_slices fed in turn on ONE stream -- they share the separator's step workspace -- with a
    ``forward`` of another length between their feeds: each returns the bits of its solo run."""
    sep = mel_seps["realtime"]
    xs = [track(1, N_TRACK).cuda(), track(1, N_TRACK + 3)[..., 3:].cuda()]
    hops = [2, 1]
    want = [run_session(sep, x, m) for x, m in zip(xs, hops)]
    other = track(1, 7 * H + 11).cuda()
    other_want = sep.forward(other).clone()
    sessions, parts = [sep.stream(1, m) for m in hops], [[], []]
    for p in range(0, N_TRACK, FEED):
        for i in (0, 1):
            parts[i].append(sessions[i].feed(xs[i][..., p:p + FEED]))
            assert torch.equal(sep.forward(other), other_want)
    for i in (0, 1):
        parts[i].append(sessions[i].flush())
        assert torch.equal(torch.cat(parts[i], dim=-1), want[i]), i
    assert not torch.equal(want[0], want[1])


def test_feed_converts_what_is_not_contiguous_fp32(mel_seps):
    """A float64 block and a block with a sample stride of 2 are the fp32 contiguous feed, bit for bit."""
    sep = mel_seps["realtime"]
    x = track(1, N_TRACK).cuda()
    want = run_session(sep, x, 2)
    wide = torch.zeros(1, 2, 2 * N_TRACK, device="cuda")
    wide[..., ::2] = x
    wide[..., 1::2] = float("nan")
    strided = wide[..., ::2]
    assert strided.stride(-1) == 2 and torch.equal(strided, x)
    assert torch.equal(run_session(sep, strided, 2), want)
    assert torch.equal(run_session(sep, x.double(), 2), want)
