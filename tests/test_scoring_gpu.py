"""Framewise and global SDR on the MI355X (xumx_slicq_amd/scoring.py, csrc/score.hip) against the definition restated in
float64 numpy (``restate`` below: per frame ``np.sum(..., dtype=float64)``, ``np.nanmedian``).

Tolerance, derived and not measured: both sides sum the same fp64 products of fp32 samples and differ in the order of the sum
alone (and in whether a square is rounded before it is added).  With at most about 1e5 terms per frame that is a relative error
of at most n * 2^-53 ~ 1e-11 in a moment, about 1e-10 dB.  The bar is TOL = 1e-9 dB absolute on every finite frame value,
median and global score; NaN and +-inf must match in position and sign.

Shapes are tiny (window 1000 mostly): the kernel's hazards sit at frame and piece edges and at misaligned rows, not at size."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9
SEP = ("bass", "vocals", "other", "drums")          # Separator.sources
DS = ("vocals", "drums", "bass", "other")           # DeviceDataset.sources


# ---- the definition, in float64 numpy -----------------------------------------------------------------------------------
def restate(est, tgt, W, silent="any", target_order=SEP, estimate_order=SEP):
    """est (4 | 5, B, 2, N), tgt (4, B, 2, N) float32 arrays -> {name: {"frames" (B, F), "sdr_median" (B,), "sdr_global" (B,)}}."""
    est, tgt = np.asarray(est), np.asarray(tgt)
    assert est.dtype == np.float32 and tgt.dtype == np.float32
    B, N = tgt.shape[1], tgt.shape[3]
    F = max(1, N // W)
    flen = W if N >= W else N
    num, den, ene = (np.zeros((4, B, F)) for _ in range(3))
    glob = np.zeros((4, B))
    for i, name in enumerate(target_order):
        j = estimate_order.index(name)
        for b in range(B):
            s, e = tgt[i, b].astype(np.float64), est[j, b].astype(np.float64)
            for f in range(F):
                sf, ef = s[:, f * flen:(f + 1) * flen], e[:, f * flen:(f + 1) * flen]
                num[i, b, f] = np.sum(sf * sf, dtype=np.float64)
                den[i, b, f] = np.sum((ef - sf) * (ef - sf), dtype=np.float64)
                ene[i, b, f] = np.sum(ef * ef, dtype=np.float64)
            glob[i, b] = 10.0 * np.log10((np.sum(s * s, dtype=np.float64) + 1e-10) / (np.sum((e - s) * (e - s), dtype=np.float64) + 1e-10))
    if silent == "any":
        quiet = np.broadcast_to(((num == 0) | (ene == 0)).any(axis=0, keepdims=True), num.shape)
    else:
        quiet = num == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        frames = np.where(quiet, np.nan, np.where(den == 0, np.inf, 10.0 * np.log10(num / np.where(den == 0, 1.0, den))))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # "All-NaN slice": the median of no frame is NaN
        med = np.nanmedian(frames, axis=2)
    return {name: {"frames": frames[i], "sdr_median": med[i], "sdr_global": glob[i]} for i, name in enumerate(target_order)}


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", got, want)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (what, "inf positions or signs", got, want)
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"[scoring] {what}: {int(fin.sum())} finite values, max |error| {err:.2e} dB")
    assert err <= TOL, (what, err)


def agrees(res, ref, what):
    assert res["metric"] == "framewise-sdr" and sorted(res["targets"]) == sorted(ref)
    for name, r in ref.items():
        g = res["targets"][name]
        assert isinstance(g["frames"], np.ndarray) and g["frames"].dtype == np.float64
        close(g["frames"], r["frames"], f"{what} {name} frames")
        close(g["sdr_median"], r["sdr_median"], f"{what} {name} median")
        close(g["sdr_global"], r["sdr_global"], f"{what} {name} global")


def bits(res):
    return {n: (r["frames"].view(np.int64).copy(), np.asarray(r["sdr_median"]).view(np.int64), np.asarray(r["sdr_global"]).view(np.int64))
            for n, r in res["targets"].items()}


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return all(all(np.array_equal(x, y) for x, y in zip(a[n], b[n])) for n in a)


def signals(N, B=2, seed=0, stems=4, noise=(0.3, 0.1, 0.03, 0.01)):
    """targets (4, B, 2, N) and estimates = targets + noise of a level per target, fp32 on the host."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randn(4, B, 2, N, generator=g)
    est = torch.randn(stems, B, 2, N, generator=g)
    for i in range(4):
        est[i] = tgt[i] + noise[i] * est[i]
    return est, tgt


@pytest.fixture(scope="module")
def track():
    """The N = 10337 track of cases 1-3, with its one-shot reference."""
    est, tgt = signals(10337, seed=1)
    return est, tgt, restate(est.numpy(), tgt.numpy(), 1000)


# ---- 1. agreement and edge frames -------------------------------------------------------------------------------------
def test_frames_medians_and_global_scores_agree_with_the_restatement(track):
    from xumx_slicq_amd.scoring import score
    est, tgt, ref = track
    res = score(est.cuda(), tgt.cuda(), window=1000)
    assert res["window"] == 1000 and res["silent"] == "any" and res["targets"]["bass"]["frames"].shape == (2, 10)
    agrees(res, ref, "N=10337")
    # the global score includes the 337-sample tail: without it the figures differ by far more than the bar
    cut = restate(est.numpy()[..., :10000], tgt.numpy()[..., :10000], 1000)
    assert max(abs(cut[n]["sdr_global"] - ref[n]["sdr_global"]).max() for n in SEP) > 1e3 * TOL


@pytest.mark.parametrize("N,frames", [(999, 1), (2000, 2), (3000, 3), (1000, 1), (1999, 1)])
def test_short_tracks_even_and_odd_frame_counts(N, frames):
    from xumx_slicq_amd.scoring import score
    est, tgt = signals(N, seed=N)
    res = score(est.cuda(), tgt.cuda(), window=1000)
    assert res["targets"]["drums"]["frames"].shape == (2, frames)
    agrees(res, restate(est.numpy(), tgt.numpy(), 1000), f"N={N}")


@pytest.mark.parametrize("est_off,tgt_off", [(0, 0), (3, 3), (1, 2), (4, 0)])
def test_rows_of_any_alignment_are_read_where_they_lie(est_off, tgt_off):
    """Views into wider tensors whose row stride is a multiple of 4 floats: equal offsets take the 16-byte path (with a scalar
    head and tail when the offset is odd), different offsets modulo 4 the 4-byte path."""
    from xumx_slicq_amd.scoring import score
    N = 10337
    est, tgt = signals(N, seed=7)
    E = torch.full((4, 2, 2, 10344), 1e6).cuda()
    T = torch.full((4, 2, 2, 10344), -1e6).cuda()
    E[..., est_off:est_off + N] = est.cuda()
    T[..., tgt_off:tgt_off + N] = tgt.cuda()
    ev, tv = E[..., est_off:est_off + N], T[..., tgt_off:tgt_off + N]
    assert not ev.is_contiguous() and ev.stride(2) == 10344
    agrees(score(ev, tv, window=1000), restate(est.numpy(), tgt.numpy(), 1000), f"offsets {est_off}/{tgt_off}")


# ---- 2. piece invariance -------------------------------------------------------------------------------------------------
def test_pieces_that_are_misaligned_views_give_the_one_shot_result(track):
    from xumx_slicq_amd.scoring import TrackScorer, score
    est, tgt, ref = track
    E, T = est.cuda(), tgt.cuda()
    cuts = [(0, 4099), (4099, 4100), (4100, 10337)]

    def run():
        sc = TrackScorer(2, 10337, window=1000)
        for a, b in cuts:
            ev, tv = E[..., a:b], T[..., a:b]
            assert ev.data_ptr() == E.data_ptr() + 4 * a and ev.stride(2) == 10337      # a view: no copy, the full row stride
            sc.add(ev, tv)
        return sc.result()

    one, first, second = score(E, T, window=1000), run(), run()
    agrees(first, ref, "three pieces")
    for n in SEP:
        for k in ("frames", "sdr_median", "sdr_global"):
            close(first["targets"][n][k], one["targets"][n][k], f"pieces vs one shot, {n} {k}")
    assert same_bits(first, second), "the same split gave different bits"
    sc = TrackScorer(2, 10337, window=1000)
    sc.add(E[..., :4099], T[..., :4099])
    with pytest.raises(ValueError, match="overlaps"):
        sc.add(E[..., 4000:5000], T[..., 4000:5000], offset=4000)
    with pytest.raises(ValueError, match="out of range"):
        sc.add(E[..., 4099:], T[..., 4099:], offset=5000)
    with pytest.raises(ValueError, match="add the rest"):
        sc.result()
    sc.add(E[..., 4099:], T[..., 4099:], offset=4099)
    agrees(sc.result(), ref, "two pieces")                  # (another split: another summation tree, within the bar all the same)


# ---- 3. silence and perfection -----------------------------------------------------------------------------------------
def test_silent_frames_perfect_frames_and_silent_targets():
    from xumx_slicq_amd.scoring import score
    est, tgt = signals(10337, B=1, seed=3)
    V, D, Bs = SEP.index("vocals"), SEP.index("drums"), SEP.index("bass")
    tgt[V, :, :, 3000:5000] = 0.0                         # the vocals reference is silent over frames 3 and 4 exactly
    est[D, :, :, 6000:7000] = 0.0                         # the drums estimate over frame 6
    est[Bs, :, :, 8000:9000] = tgt[Bs, :, :, 8000:9000]   # a perfect bass frame
    E, T = est.cuda(), tgt.cuda()
    res_any, res_own = score(E, T, window=1000), score(E, T, window=1000, silent="own")
    agrees(res_any, restate(est.numpy(), tgt.numpy(), 1000, "any"), "silent=any")
    agrees(res_own, restate(est.numpy(), tgt.numpy(), 1000, "own"), "silent=own")
    for n in SEP:
        fa, fo = res_any["targets"][n]["frames"][0], res_own["targets"][n]["frames"][0]
        assert np.isnan(fa[[3, 4, 6]]).all() and np.isnan(fa).sum() == 3, n
        assert np.array_equal(np.flatnonzero(np.isnan(fo)), [3, 4] if n == "vocals" else []), n
    assert res_any["targets"]["bass"]["frames"][0, 8] == np.inf and res_own["targets"]["bass"]["frames"][0, 8] == np.inf
    assert abs(res_own["targets"]["drums"]["frames"][0, 6]) < TOL           # estimate 0: den == num, 0 dB
    # +inf sorts last: the median of seven frames, one of them +inf, is the fourth smallest finite value
    fin = np.sort(res_any["targets"]["bass"]["frames"][0][np.isfinite(res_any["targets"]["bass"]["frames"][0])])
    assert len(fin) == 6 and res_any["targets"]["bass"]["sdr_median"][0] == fin[3]
    # a target silent in every frame
    tgt[SEP.index("other")] = 0.0
    T = tgt.cuda()
    own, joint = score(E, T, window=1000, silent="own"), score(E, T, window=1000)
    agrees(own, restate(est.numpy(), tgt.numpy(), 1000, "own"), "silent target, own")
    agrees(joint, restate(est.numpy(), tgt.numpy(), 1000, "any"), "silent target, any")
    assert np.isnan(own["targets"]["other"]["sdr_median"][0]) and np.isfinite(own["targets"]["other"]["sdr_global"][0])
    assert np.isfinite(own["targets"]["bass"]["sdr_median"][0])
    assert all(np.isnan(joint["targets"][n]["sdr_median"][0]) for n in SEP)


def test_an_estimate_twice_the_reference_is_not_silent():
    """s_hat = 2 s gives den == num exactly, as s_hat = 0 does: the joint rule must look at the estimate's own energy."""
    from xumx_slicq_amd.scoring import score
    est, tgt = signals(3000, B=1, seed=5)
    est[2, :, :, 1000:2000] = 2.0 * tgt[2, :, :, 1000:2000]
    res = score(est.cuda(), tgt.cuda(), window=1000)
    agrees(res, restate(est.numpy(), tgt.numpy(), 1000), "s_hat = 2 s")
    assert not np.isnan(res["targets"]["bass"]["frames"]).any() and abs(res["targets"]["other"]["frames"][0, 1]) < TOL


# ---- 4. name mapping ---------------------------------------------------------------------------------------------------------
def test_targets_are_matched_by_name_not_by_position():
    from xumx_slicq_amd.scoring import score
    N = 5000
    g = torch.Generator().manual_seed(11)
    level = {"bass": 0.5, "vocals": 0.2, "other": 0.05, "drums": 0.01}        # 8, 12 and 14 dB apart
    named = {n: torch.randn(2, 2, N, generator=g) for n in SEP}
    tgt = torch.stack([named[n] for n in DS])                                  # the dataset's column order
    est = torch.stack([named[n] + level[n] * torch.randn(2, 2, N, generator=g) for n in SEP])
    res = score(est.cuda(), tgt.cuda(), window=1000, target_order=DS)
    ref = restate(est.numpy(), tgt.numpy(), 1000, target_order=DS)
    agrees(res, ref, "dataset order")
    for n in SEP:
        want = -20.0 * np.log10(level[n])
        assert abs(res["targets"][n]["sdr_median"][0] - want) < 1.0 and abs(res["targets"][n]["sdr_global"][1] - want) < 1.0, n
    with pytest.raises(ValueError, match="unknown target"):
        score(est.cuda(), tgt.cuda(), window=1000, target_order=("vocals", "drums", "bass", "piano"))


# ---- 5. the real window ------------------------------------------------------------------------------------------------------
def test_one_second_frames_at_44100():
    from xumx_slicq_amd.scoring import score
    N = 3 * 44100 + 12345
    est, tgt = signals(N, B=1, seed=13)
    res = score(est.cuda(), tgt.cuda())
    assert res["window"] == 44100 and res["targets"]["vocals"]["frames"].shape == (1, 3)
    agrees(res, restate(est.numpy(), tgt.numpy(), 44100), "W=44100")


# ---- 6. residual -----------------------------------------------------------------------------------------------------------
def test_a_fifth_stem_is_ignored(track):
    from xumx_slicq_amd.scoring import score
    est, tgt, ref = track
    five = torch.cat([est, 100.0 * torch.ones(1, 2, 2, 10337)], dim=0)
    res = score(five.cuda(), tgt.cuda(), window=1000)
    agrees(res, ref, "five stems")
    assert same_bits(res, score(est.cuda(), tgt.cuda(), window=1000))


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
CS, W_E2E = 30000, 7000                        # chunk size (S = 5 slices), not a multiple of the window
LENGTHS = (int(1.5 * CS) + 123, int(2.5 * CS) + 77)


@pytest.fixture(scope="module")
def stems():
    from xumx_slicq_amd.synth import synth_audio
    out = []
    for t, n in enumerate(LENGTHS):
        out.append({s: (0.25 * synth_audio(n, seed=700 + 10 * t + k)[0]).numpy() for k, s in enumerate(DS)})
    return out


def _expected(sep, ds, i, W):
    est, tgt = [], []
    for x, y in ds.pieces(i, sep.chunk_size):
        est.append(sep(x).cpu())
        tgt.append(y.cpu())
    return restate(torch.cat(est, dim=-1).numpy(), torch.cat(tgt, dim=-1).numpy(), W, target_order=ds.targets, estimate_order=tuple(sep.sources))


@pytest.mark.parametrize("wiener", [False, True], ids=["mixphase", "wiener"])
def test_evaluate_dataset_end_to_end(stems, wiener, tmp_path):
    from xumx_slicq_amd import evaluation
    from xumx_slicq_amd.audio import save_wav_float
    from xumx_slicq_amd.data import DeviceDataset
    from xumx_slicq_amd.separator import seeded_separator
    ds = DeviceDataset.from_arrays(stems, storage="fp32", names=["short", "long"])
    sep = seeded_separator(realtime=False, wiener=wiener, chunk_size=CS)
    assert CS % W_E2E and [len(list(ds.pieces(i, CS))) for i in (0, 1)] == [2, 3]
    out = evaluation.evaluate_dataset(sep, ds, window=W_E2E)
    assert out["metric"] == "framewise-sdr" and out["window"] == W_E2E and list(out["tracks"]) == ["short", "long"]
    for i, name in enumerate(ds.names):
        agrees(out["tracks"][name], _expected(sep, ds, i, W_E2E), f"{name} wiener={wiener}")
    for t in SEP:
        med = [out["tracks"][n]["targets"][t]["sdr_median"][0] for n in ds.names]
        glo = [out["tracks"][n]["targets"][t]["sdr_global"][0] for n in ds.names]
        a = out["aggregate"][t]
        assert a["sdr_median"] == np.median(med) and a["sdr_global_mean"] == np.mean(glo) and a["sdr_global_median"] == np.median(glo)
    only = evaluation.evaluate_dataset(sep, ds, tracks=["long"], window=W_E2E, silent="own")
    assert list(only["tracks"]) == ["long"] and only["silent"] == "own"
    if not wiener:
        return
    # the command line over the same stems written with the project's wav writer: the default Separator (Wiener-EM, the default
    # chunk size, so each track is one piece)
    for name, tr in zip(ds.names, stems):
        os.makedirs(tmp_path / "root" / name)
        for s in DS:
            save_wav_float(str(tmp_path / "root" / name / f"{s}.wav"), torch.from_numpy(tr[s]), 44100)
    agg = evaluation.evaluation_main(["--root", str(tmp_path / "root"), "--out", str(tmp_path / "out"), "--window-seconds", str(W_E2E / 44100.0)])
    sep.chunk_size = 2621440
    want = evaluation.evaluate_dataset(sep, ds, window=W_E2E)
    assert agg["window"] == W_E2E and sorted(os.listdir(tmp_path / "out")) == ["aggregate.json", "long.json", "short.json"]
    on_disk = json.load(open(tmp_path / "out" / "aggregate.json"))
    assert on_disk["metric"] == "framewise-sdr" and on_disk["tracks"] == ["long", "short"]
    for t in SEP:
        assert on_disk["aggregate"][t] == want["aggregate"][t] == agg["aggregate"][t]
    for name in ds.names:
        got = json.load(open(tmp_path / "out" / f"{name}.json"))
        assert got["track"] == name and got["window"] == W_E2E and got["silent"] == "any"
        for t in SEP:
            w = want["tracks"][name]["targets"][t]
            assert got["targets"][t]["sdr_median"] == w["sdr_median"] and got["targets"][t]["sdr_global"] == w["sdr_global"]
            assert got["targets"][t]["frames"] == w["frames"].tolist()          # (no NaN or inf in these tracks)


# ---- 8. the stream contract ------------------------------------------------------------------------------------------------
def test_score_on_a_side_stream_behind_a_delayed_producer(track):
    """The inputs are produced on a non-default stream behind a device-side delay and overwritten with a decoy behind the call,
    with no synchronisation in between: a launch on any other stream reads the decoy or unwritten memory."""
    from xumx_slicq_amd.scoring import TrackScorer, score
    est, tgt, ref = track
    E0, T0 = est.cuda(), tgt.cuda()
    want = score(E0, T0, window=1000)
    want_pieces = TrackScorer(2, 10337, window=1000).add(E0[..., :4099], T0[..., :4099]).add(E0[..., 4099:], T0[..., 4099:]).result()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    E, T = torch.full_like(E0, 3.0), torch.full_like(T0, -5.0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(1_000_000)
    b.record()
    b.synchronize()
    per_ms = 1_000_000 / max(a.elapsed_time(b), 1e-3)      # units of the spin per millisecond, measured: no hard-coded clock rate
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(100.0 * per_ms))             # 100 ms: far longer than the host needs to enqueue what follows
        delay = torch.cuda.Event()
        delay.record(s)
        E.copy_(E0)
        T.copy_(T0)
        sc = TrackScorer(2, 10337, window=1000).add(E[..., :4099], T[..., :4099]).add(E[..., 4099:], T[..., 4099:])
        whole = TrackScorer(2, 10337, window=1000).add(E, T)           # what score() does, without its read-back
        E.fill_(3.0)
        T.fill_(-5.0)
        pending = not delay.query()                        # everything up to here was enqueued while the producer was still delayed
        got, got_pieces = whole.result(), sc.result()      # (result() reads back: it waits for the stream)
        again = score(E0, T0, window=1000)
    s.synchronize()
    assert pending, "the delay had ended before the pieces were enqueued: this run proved nothing"
    assert same_bits(got, want) and same_bits(got_pieces, want_pieces) and same_bits(again, want)
    agrees(got, ref, "side stream")
    torch.cuda.synchronize()
