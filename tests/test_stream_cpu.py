"""The streaming session without a GPU: the step schedule on the absolute block grid (xsq_stream_schedule, ``StreamGrid``), the
schedule spelled through the CPU oracle (``streamed_loop`` over ``oracle.separator.separate`` equals one ``separate`` of the whole
signal, and does not when the window is one slice short), the dependency window of a mask that the constants of the code and
DESIGN.md 4.11 state, and what ``Separator.stream`` and the CLI refuse.  The GPU half is tests/test_stream_gpu.py.  For the product
plan, Bark-262: the same window in every one of its 70 blocks and the same loop over the oracle; for the stage tests of
tests/test_stream_stages_gpu.py: the slice-shift property of the float64 transforms their references rest on, and the rule behind
their bounds on the committed table.
"""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from oracle import model as omodel
from oracle import separator as osep
from oracle import slicqt as O
from test_ref64_mel_cpu import make_mel_plan, make_mel_sd, one_thread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2016                    # the Mel-32 plan
H = L // 4
N_TRACK = 23 * H + 17       # S = 13 slices, 12 blocks, the last one 521 samples
LENGTHS = sorted({1, L // 2, L // 2 + 1, 2 * H, 2 * H + 1, N_TRACK, 40 * H})


@pytest.fixture(scope="module")
def plan():
    p = make_mel_plan()
    assert p.L == L
    return p


@pytest.fixture(scope="module")
def sd(plan):
    return make_mel_sd(plan)


def track(nb=1, n=N_TRACK):
    return 2 * torch.rand(nb, 2, n, generator=torch.Generator().manual_seed(20261019)) - 1


def slices_of(n):
    return ((max(n, L // 2 + 1) + H - 1) // H + 1) // 2 + 1


# ---- the schedule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back", [2, 3])
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("N", LENGTHS)
def test_every_block_is_emitted_once_in_order_on_its_full_window(N, m, back):
    from xumx_slicq_amd.separator import STREAM_AHEAD, stream_steps, stream_trigger
    steps = stream_steps(N, L, m, back)
    S, nblk = slices_of(N), -(-N // (2 * H))
    assert [b for b0, k, *_ in steps for b in range(b0, b0 + k)] == list(range(nblk))
    inverted = []
    for j, (b0, k, first, w0, w1, trigger) in enumerate(steps):
        assert b0 == j * m and 1 <= k <= m and first == (0 if j == 0 else b0 + 1)
        last = b0 + k                                   # block b needs the slices b and b + 1
        inverted += list(range(first, last + 1))
        assert w1 == min(S - 1, last + STREAM_AHEAD), "every slice ahead that the signal has"
        assert w0 <= max(0, first - back), "every slice behind that the signal has"
        assert w0 == max(0, min(first - back, w1 - 2)) and w1 - w0 + 1 >= 3, "and no more, but the 3 the conv stack needs"
        assert trigger == stream_trigger(j, L, m) == (2 * (j + 1) * m + 6) * H
    assert inverted == list(range(nblk + 1)), "no slice is inverted twice"


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("N", LENGTHS)
def test_the_steps_do_not_depend_on_the_partition_into_feeds(N, m):
    from xumx_slicq_amd.separator import StreamGrid, stream_steps
    want = stream_steps(N, L, m, 3)
    gen = torch.Generator().manual_seed(N + m)
    parts = [[N], [1, N - 1], [700] * (N // 700) + [N % 700], [2 * H] * (N // (2 * H)) + [N % (2 * H)], [N // 2, 0, N - N // 2]]
    cuts = sorted(torch.randint(0, N + 1, (5,), generator=gen).tolist())
    parts.append([b - a for a, b in zip([0] + cuts, cuts + [N])])
    for feeds in parts:
        assert sum(feeds) == N
        grid, fired = StreamGrid(L, m, 3), []
        for n in feeds:
            events = grid.feed(n)
            assert sum(c for c, _ in events) == n and all(c >= 1 for c, _ in events)
            fired += [step for _, step in events if step is not None]
        assert grid.samples_in == N
        # what fired while the stream was open is the head of the list, with the same windows: the clipping at the end binds later only
        assert fired == list(range(len(fired))) and all(want[j][5] <= N for j in fired)
        assert len(fired) == sum(1 for s in want if s[5] <= N)
        assert stream_steps(N + 100 * L, L, m, 3)[:len(fired)] == want[:len(fired)]
        assert grid.flush() == want[len(fired):], feeds


def test_latency_is_two_slice_lengths_from_the_first_sample_of_a_block():
    from xumx_slicq_amd.separator import stream_trigger
    for k in range(5):
        assert stream_trigger(k, L, 1) - 2 * k * H == 8 * H == 2 * L
    assert 8 * (18060 // 4) == 36120 and 8 * H == 4032          # Bark-262: 0.82 s at 44.1 kHz; Mel-32: 91 ms


def test_c_schedule_refuses_bad_arguments():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import stream_steps
    sched = _lib.lib.xsq_stream_schedule
    assert sched(0, L, 1, 3, 2, None, 0) == 0
    for args in ((-1, L, 1, 3, 2), (100, 0, 1, 3, 2), (100, 2018, 1, 3, 2), (100, L, 0, 3, 2), (100, L, 1, -1, 2), (100, L, 1, 3, -1)):
        assert sched(*args, None, 0) < 0, args
    with pytest.raises(ValueError):
        stream_steps(100, L, 0, 3)
    for fn, args in ((_lib.lib.xsq_stream_create, (None, None, None, 1, 1, 3, 2)), (_lib.lib.xsq_stream_push, (None, None, None, 1, 1, None)),
                     (_lib.lib.xsq_stream_step, (None, None, None, None, 1, 0, -1, None, 1, 1, None, 0, None))):
        assert fn(*args) != 0
    assert _lib.lib.xsq_stream_state_bytes(None) == 0 and _lib.lib.xsq_stream_workspace(None, None) == 0


# ---- streamed_loop over the oracle ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(plan, sd):
    x = track()
    with one_thread():
        return x, {causal: osep.separate(plan, sd, x, causal=causal, wiener=False) for causal in (True, False)}


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("causal", [True, False])
def test_streamed_loop_over_the_oracle_is_one_separate_of_the_whole(plan, sd, whole, causal, m):
    """Measured: 0.0 at the full window for both stacks; one slice short 0.035 (causal) and 0.056 (offline) max against a signal RMS of
    0.32 -- the 1e-6 only leaves room for another torch build, the 1e-3 keeps it from being vacuous."""
    from xumx_slicq_amd.separator import STREAM_BACK, streamed_loop
    x, ref = whole
    back = STREAM_BACK[causal]
    calls = []

    def forward(a):
        calls.append(a.shape[-1])
        return osep.separate(plan, sd, a, causal=causal, wiener=False)

    with one_thread():
        full = streamed_loop(forward, x, L, m, back)
        ncalls = len(calls)
        short = streamed_loop(forward, x, L, m, back - 1)
    assert ncalls == -(-12 // m) and max(calls[:ncalls]) <= (2 * (m + back + 2 + 2) + 2) * H
    assert full.shape == ref[causal].shape == (4, 1, 2, N_TRACK)
    e_full, e_short = float((full - ref[causal]).abs().max()), float((short - ref[causal]).abs().max())
    print(f"causal={causal} m={m}: max error full window {e_full:.3g}, one slice short {e_short:.3g}")
    assert e_full <= 1e-6
    assert e_short > 1e-3


# ---- the dependency window ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_the_dependency_window_is_what_the_constants_and_the_design_say(plan, sd, causal):
    """Perturbing the magnitudes of slice k moves the masks of the slices k - 2 .. k + back exactly, in every one of the 23 blocks
    together: the mask of slice s reads the slices s - back .. s + 2."""
    from xumx_slicq_amd.separator import STREAM_AHEAD, STREAM_BACK
    k = 6
    with one_thread(), torch.no_grad():
        X = O.forward(plan, track())
        touched = set()
        for b, Xb in enumerate(X):
            mag = omodel.abs_of_real_complex(Xb)
            assert mag.shape[3] == 13
            base = omodel.cdae_masks(sd, b, mag, causal)
            mag2 = mag.clone()
            mag2[:, :, :, k] *= 1.5
            moved = (omodel.cdae_masks(sd, b, mag2, causal) != base).any(-1).flatten(0, 3).any(0)        # per slice
            touched |= {s for s in range(13) if bool(moved[s])}
    back, ahead = STREAM_BACK[causal], STREAM_AHEAD
    assert touched == set(range(k - ahead, k + back + 1)), sorted(touched)
    assert (back, ahead) == ((3, 2) if causal else (2, 2))
    header = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    name = "XSQ_STREAM_BACK_CAUSAL" if causal else "XSQ_STREAM_BACK_OFFLINE"
    assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == back
    assert int(re.search(r"#define XSQ_STREAM_AHEAD (\d+)", header).group(1)) == ahead
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.11"):]
    assert f"`s - {back} .. s + {ahead}`" in section


# ---- Bark-262: the product plan, the only one with frequency taps --------------------------------------------------------------
BARK_L = 18060
BARK_N = 100000             # S = 13 slices, 12 blocks, the last one 670 samples


def bark_track():
    return 2 * torch.rand(1, 2, BARK_N, generator=torch.Generator().manual_seed(20261020)) - 1


@pytest.mark.parametrize("causal", [True, False])
def test_the_dependency_window_on_bark_holds_in_every_block(oracle_plan, seeded_sd, causal):
    """The perturbation of the Mel test on the 70 blocks of Bark-262 (kernels of 3 and 5 bands in frequency): slice k moves the
    masks of the slices k - 2 .. k + back in EVERY block, not only in their union -- no block has a shorter or a longer reach."""
    from xumx_slicq_amd.separator import STREAM_AHEAD, STREAM_BACK
    k = 6
    assert oracle_plan.L == BARK_L and oracle_plan.nslices(BARK_N) == 13 and len(oracle_plan.blocks) == 70
    want = set(range(k - STREAM_AHEAD, k + STREAM_BACK[causal] + 1))
    with one_thread(), torch.no_grad():
        X = O.forward(oracle_plan, bark_track())
        touched, odd = set(), []
        for b, Xb in enumerate(X):
            mag = omodel.abs_of_real_complex(Xb)
            assert mag.shape[3] == 13
            base = omodel.cdae_masks(seeded_sd, b, mag, causal)
            mag2 = mag.clone()
            mag2[:, :, :, k] *= 1.5
            moved = (omodel.cdae_masks(seeded_sd, b, mag2, causal) != base).any(-1).flatten(0, 3).any(0)
            mine = {s for s in range(13) if bool(moved[s])}
            touched |= mine
            if mine != want:
                odd.append((b, sorted(mine)))
    assert not odd, odd
    assert touched == want, sorted(touched)


@pytest.fixture(scope="module")
def bark_whole(oracle_plan, seeded_sd):
    x = bark_track()
    with one_thread():
        return x, {causal: osep.separate(oracle_plan, seeded_sd, x, causal=causal, wiener=False) for causal in (True, False)}


@pytest.mark.parametrize("causal", [True, False])
def test_streamed_loop_over_the_oracle_on_bark(oracle_plan, seeded_sd, bark_whole, causal):
    """m = 3: four steps over the 12 blocks, the last clipped at the signal.  The bounds are those of the Mel test."""
    from xumx_slicq_amd.separator import STREAM_BACK, streamed_loop
    x, ref = bark_whole
    back, m, h = STREAM_BACK[causal], 3, BARK_L // 4
    calls = []

    def forward(a):
        calls.append(a.shape[-1])
        return osep.separate(oracle_plan, seeded_sd, a, causal=causal, wiener=False)

    with one_thread():
        full = streamed_loop(forward, x, BARK_L, m, back)
        ncalls = len(calls)
        short = streamed_loop(forward, x, BARK_L, m, back - 1)
    assert ncalls == 4 and max(calls[:ncalls]) <= (2 * (m + back + 2 + 2) + 2) * h
    assert full.shape == ref[causal].shape == (4, 1, 2, BARK_N)
    e_full, e_short = float((full - ref[causal]).abs().max()), float((short - ref[causal]).abs().max())
    print(f"bark causal={causal} m={m}: max error full window {e_full:.3g}, one slice short {e_short:.3g}")
    assert e_full <= 1e-6
    assert e_short > 1e-3


# ---- what the stage tests of tests/test_stream_stages_gpu.py rest on ------------------------------------------------------------
@pytest.mark.parametrize("which", ["mel", "bark"])
def test_slices_of_the_float64_transforms_do_not_depend_on_where_the_signal_starts(plan, oracle_plan, which):
    """A slice is a function of its own 4h samples, and an inverted slice adds to its own 4h samples: (a) the slices 1 .. S of
    ``ref64.forward(v)``, v of (2S + 2)h samples, are the slices k + 1 .. k + S of any signal that holds v from sample 2hk on;
    (b) the overlap-add of ``ref64.inverse`` over consecutive slice ranges is ``ref64.inverse`` of all the slices, and the blocks
    a range closes on its own are that span of the whole.  Float64: 1e-13 of the RMS."""
    from oracle import ref64
    p = plan if which == "mel" else oracle_plan
    h, S, gen = p.h, 3, torch.Generator().manual_seed(p.L)
    v = 2 * torch.rand(2, (2 * S + 2) * h, generator=gen, dtype=torch.float64) - 1
    own = ref64.forward(p, v)
    assert own[0].shape[-3] == S + 2
    for k, tail in ((1, 0), (2, 3 * h + 5)):
        w = torch.cat([torch.randn(2, 2 * h * k, generator=gen, dtype=torch.float64), v,
                       torch.randn(2, tail, generator=gen, dtype=torch.float64)], dim=-1)
        for a, b in zip(own, ref64.forward(p, w)):
            a, b = a[..., 1:S + 1, :, :], b[..., k + 1:k + S + 1, :, :]
            assert float((a - b).abs().max()) <= 1e-13 * float(b.pow(2).mean().sqrt()), (which, k)
    S_tot = 9
    X = [torch.randn(2, F, S_tot, T, 2, generator=gen, dtype=torch.float64) for (_, F, T) in p.blocks]
    length = 2 * S_tot * h
    whole = ref64.inverse(p, X, length)
    rms = float(whole.pow(2).mean().sqrt())
    for parts in ((9,), (4, 3, 2), (2, 7), (2, 1, 1, 1, 1, 1, 1, 1)):
        pad, a = torch.zeros(2, (2 * S_tot + 2) * h, dtype=torch.float64), 0
        for n in parts:
            # a zero slice in front: the range's own first half is then part of what inverse returns
            seg = ref64.inverse(p, [torch.cat([torch.zeros_like(x[..., :1, :, :]), x[..., a:a + n, :, :]], dim=-3) for x in X], (2 * n + 2) * h)
            pad[:, 2 * a * h:(2 * a + 2 * n + 2) * h] += seg
            if n >= 2:       # the blocks a .. a + n - 2 lie inside the range
                alone = ref64.inverse(p, [x[..., a:a + n, :, :] for x in X], 2 * (n - 1) * h)
                assert float((alone - whole[:, 2 * a * h:2 * (a + n - 1) * h]).abs().max()) <= 1e-13 * rms, (which, parts, a)
            a += n
        assert a == S_tot and float((pad[:, 2 * h:2 * h + length] - whole).abs().max()) <= 1e-13 * rms, (which, parts)


def test_every_stage_bound_follows_the_rule_from_the_committed_table():
    """M of tests/test_stream_stages_gpu.py = the smallest power of two that is at least twice the worst e_gpu / E of
    profiles/stream_stage_parity.json (measured on MI355X), at most M_CAP; the table covers both plans and every partition."""
    import json
    from oracle.parity import M_CAP
    from test_stream_stages_gpu import M, PARTITIONS, PLANS
    table = json.load(open(os.path.join(ROOT, "profiles", "stream_stage_parity.json")))
    for stage, bound in M.items():
        worst = table["M"][stage]["worst_ratio"]
        want = 1
        while want < 2 * worst:
            want *= 2
        assert 0 < worst and bound == min(want, M_CAP) and table["M"][stage]["M"] == bound, (stage, worst, bound)
        cases = table["tables"][stage]
        assert all(any(c.startswith(name) for c in cases) for name in PLANS)
        assert max(rec["worst_ratio"] for rec in cases.values()) == worst
    for name in PLANS:
        for B in (1, 2):
            assert all(f"{name} B={B} partition {parts}" in table["tables"]["inverse_carry"] for parts in PARTITIONS)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _stub(realtime=(True,), causal=(True,), **options):
    from xumx_slicq_amd.separator import Separator

    class Stub(Separator):                    # the refusals come before any device work
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.xumx_model = SimpleNamespace(sliced_umx=[SimpleNamespace(realtime=r, causal=c) for r, c in zip(realtime, causal)], **options)

    return Stub()


def test_stream_refuses_what_cannot_stream():
    from xumx_slicq_amd import StreamSession, streamed_loop
    from xumx_slicq_amd._lib import XsqError
    from xumx_slicq_amd.separator import StreamSession as S2
    assert StreamSession is S2 and callable(streamed_loop)
    for sep, kw, word in ((_stub(), dict(hop_slices=0), "hop_slices"), (_stub(), dict(hop_slices=-3), "hop_slices"),
                          (_stub(), dict(nb_samples=0), "nb_samples"),
                          (_stub(realtime=(False,), causal=(False,), niter=1), {}, "Wiener-EM"),
                          (_stub(realtime=(False,), causal=(False,)), {}, "Wiener-EM"),              # (the model's default is one iteration)
                          (_stub(realtime=(False,), causal=(False,), niter=3), {}, "Wiener-EM"),
                          (_stub(realtime=(False,), causal=(False,), niter=0, softmask=True), {}, "softmask"),
                          (_stub(realtime=(False,), causal=(False,), niter=0, residual=True), {}, "residual"),
                          (_stub(softmask=True), {}, "softmask"),
                          (_stub(realtime=(True, False), causal=(True, True)), {}, "mixed"),
                          (_stub(realtime=(True, True), causal=(True, False)), {}, "mixed")):
        with pytest.raises(XsqError, match=word):
            sep.stream(**kw)
    with pytest.raises(ValueError):
        streamed_loop(lambda a: a, torch.zeros(1, 2, 0), L, 1, 3)


def test_cli_refuses_stream_with_what_it_cannot_serve(capsys):
    from xumx_slicq_amd.inference import cli_parser, inference_main, parse_args
    p = cli_parser()
    a = parse_args(p, ["--stream", "4096", "--realtime"])
    assert (a.stream, a.hop_slices) == (4096, None)
    a = parse_args(p, ["--stream", "700", "--hop-slices", "4", "--niter", "0"])
    assert (a.stream, a.hop_slices, a.niter) == (700, 4, 0)
    for argv, word in ((["--stream", "4096", "--realtime", "--remix", "karaoke:vocals=0"], "--remix"),
                       (["--stream", "4096", "--realtime", "--segment", "5"], "--segment"),
                       (["--stream", "4096", "--realtime", "--overlap", "0.1"], "--segment"),
                       (["--stream", "4096"], "--niter"), (["--stream", "4096", "--niter", "1"], "--niter"),
                       (["--stream", "4096", "--niter", "2"], "--niter"),
                       (["--stream", "4096", "--niter", "0", "--softmask"], "--softmask"),
                       (["--stream", "4096", "--niter", "0", "--residual"], "--residual"),
                       (["--stream", "0", "--realtime"], "--stream"), (["--stream", "4096", "--realtime", "--hop-slices", "0"], "--hop-slices"),
                       (["--hop-slices", "2"], "--stream")):
        with pytest.raises(SystemExit) as e:
            inference_main(argv + ["--device", "cpu"])
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
