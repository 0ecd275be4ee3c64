"""Host side of the on-device scores (xumx_slicq_amd/scoring.py, evaluation.py, csrc/score.hip): frame arithmetic, refusals by
message, the command line's arguments, the shape of the JSON, and the new symbols.  What the kernels compute is held on the
GPU (tests/test_scoring_gpu.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch


# ---- frame count and tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,W,want", [(10337, 1000, (10, 1000, 337)), (999, 1000, (1, 999, 0)), (2000, 1000, (2, 1000, 0)),
                                      (3000, 1000, (3, 1000, 0)), (1000, 1000, (1, 1000, 0)), (1999, 1000, (1, 1000, 999)),
                                      (3 * 44100 + 12345, 44100, (3, 44100, 12345)), (240 * 44100, 44100, (240, 44100, 0))])
def test_frame_count_and_tail(N, W, want):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.scoring import frame_layout
    assert frame_layout(N, W) == want
    tb, wb = C.c_size_t(0), C.c_size_t(0)
    assert _lib.lib.xsq_score_workspace(2, N, W, C.byref(tb), C.byref(wb)) == 0, _lib.last_error()
    assert tb.value == 4 * 2 * (want[0] + 1) * 3 * 8                       # (4, B, F + 1, 2) moments + (4, B, F + 1) estimate energies
    slots = (want[0] + 1) * -(-want[1] // 2048)                            # every cell in slots of 2048 samples, 12 partials each
    assert wb.value == -(-2 * slots * 12 * 8 // 256) * 256


def test_default_window_is_one_second_and_the_hop_is_the_window():
    from xumx_slicq_amd.scoring import window_samples
    assert window_samples(None) == 44100 and window_samples(None, 48000.0) == 48000 and window_samples(1000, hop=1000) == 1000
    with pytest.raises(ValueError, match="hop 500 != window 1000"):
        window_samples(1000, hop=500)
    with pytest.raises(ValueError, match="at least one sample"):
        window_samples(0)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.scoring import TrackScorer, max_frames, score, target_permutation
    e, t = torch.zeros(4, 1, 2, 100), torch.zeros(4, 1, 2, 100)
    with pytest.raises(_lib.XsqError, match="no CPU fallback"):
        score(e, t, window=10)
    for bad_e, bad_t in ((torch.zeros(3, 1, 2, 100), t), (torch.zeros(4, 2, 100), t), (e, torch.zeros(5, 1, 2, 100)),
                         (e, torch.zeros(4, 1, 2, 99)), (torch.zeros(4, 1, 1, 100), torch.zeros(4, 1, 1, 100)), (e, "targets")):
        with pytest.raises(ValueError, match=r"expected estimates \(4 \| 5, B, 2, n\) and targets \(4, B, 2, n\)"):
            score(bad_e, bad_t, window=10)
    with pytest.raises(ValueError, match="hop 5 != window 10"):
        TrackScorer(1, 100, window=10, hop=5)
    with pytest.raises(ValueError, match="silent 'some'"):
        TrackScorer(1, 100, window=10, silent="some")
    with pytest.raises(ValueError, match=r"unknown target\(s\) \['piano'\]"):
        TrackScorer(1, 100, window=10, target_order=("vocals", "drums", "bass", "piano"))
    with pytest.raises(ValueError, match="four different targets"):
        target_permutation(("vocals", "vocals", "bass", "other"))
    assert max_frames() == 4096
    with pytest.raises(_lib.XsqError, match=r"4097 frames of 10 samples; the median is a sort in LDS and holds at most 4096 frames"):
        TrackScorer(1, 40970, window=10)
    with pytest.raises(_lib.XsqError, match="no CPU fallback"):
        TrackScorer(1, 100, window=10, device="cpu")


def test_name_mapping_is_a_permutation_by_name():
    from xumx_slicq_amd.data import DeviceDataset
    from xumx_slicq_amd.scoring import target_permutation
    from xumx_slicq_amd.separator import Separator
    assert tuple(Separator.sources) == ("bass", "vocals", "other", "drums") and DeviceDataset.sources == ("vocals", "drums", "bass", "other")
    assert target_permutation(DeviceDataset.sources, Separator.sources) == (1, 3, 0, 2)
    assert target_permutation(DeviceDataset.targets, Separator.sources) == (0, 1, 2, 3)
    assert target_permutation(Separator.sources, Separator.sources + ["residual"]) == (0, 1, 2, 3)


def test_c_abi_refuses_bad_arguments_with_a_message():
    from xumx_slicq_amd import _lib
    lib = _lib.lib
    tb, wb = C.c_size_t(7), C.c_size_t(7)
    assert lib.xsq_score_workspace(1, 100, 10, None, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_score_workspace(0, 100, 10, C.byref(tb), C.byref(wb)) < 0 and "B=0" in _lib.last_error() and tb.value == wb.value == 0
    assert lib.xsq_score_workspace(1, 100, 0, C.byref(tb), C.byref(wb)) < 0 and "W=0" in _lib.last_error()
    assert lib.xsq_score_workspace(1, 4097 * 10, 10, C.byref(tb), C.byref(wb)) < 0 and "at most 4096 frames" in _lib.last_error()
    assert lib.xsq_score_accumulate(None, None, None, 1, 10, 10, 10, 0, 100, 10, None, None, 0, None) < 0 and "null" in _lib.last_error()
    assert lib.xsq_score_finalise(None, 1, 10, 0, None, None, None) < 0 and "null" in _lib.last_error()
    # argument checks that come before any launch: fake non-null pointers are never dereferenced on these paths
    perm = (C.c_int * 4)(0, 1, 2, 3)
    p = C.cast(perm, C.c_void_p)
    assert lib.xsq_score_accumulate(p, p, p, 1, 50, 50, 50, 60, 100, 10, p, p, 1 << 20, None) < 0 and "piece [60, +50)" in _lib.last_error()
    assert lib.xsq_score_accumulate(p, p, p, 1, 50, 40, 50, 0, 100, 10, p, p, 1 << 20, None) < 0 and "row strides" in _lib.last_error()
    bad = (C.c_int * 4)(0, 1, 1, 3)
    assert lib.xsq_score_accumulate(p, p, C.cast(bad, C.c_void_p), 1, 50, 50, 50, 0, 100, 10, p, p, 1 << 20, None) < 0
    assert "four different stems" in _lib.last_error()
    assert lib.xsq_score_accumulate(p, p, p, 1, 50, 50, 50, 0, 100, 10, p, p, 8, None) < 0 and "workspace too small" in _lib.last_error()
    assert lib.xsq_score_finalise(p, 1, 5000, 0, p, p, None) < 0 and "at most 4096 frames" in _lib.last_error()
    assert lib.xsq_score_finalise(p, 1, 10, 2, p, p, None) < 0 and "silent_mode 2" in _lib.last_error()


# ---- command line --------------------------------------------------------------------------------------------------------
def test_command_line_arguments():
    from xumx_slicq_amd import evaluation as E
    p = E.cli_parser()
    a = E.parse_args(p, ["--root", "musdb/test", "--out", "scores"])
    assert (a.root, a.out, a.tracks, a.model_path, a.realtime, a.niter, a.softmask, a.window_seconds, a.silent) == \
        ("musdb/test", "scores", None, None, False, None, False, 1.0, "any")
    a = E.parse_args(p, ["--root", "r", "--out", "o", "--tracks", "A - B,C", "--model-path", "m", "--niter", "2", "--softmask",
                         "--window-seconds", "0.5", "--silent", "own"])
    assert (a.tracks, a.model_path, a.niter, a.softmask, a.window_seconds, a.silent) == (["A - B", "C"], "m", 2, True, 0.5, "own")
    assert E.parse_args(p, ["--root", "r", "--out", "o", "--realtime"]).realtime is True
    for argv in (["--out", "o"], ["--root", "r"], ["--root", "r", "--out", "o", "--silent", "some"],
                 ["--root", "r", "--out", "o", "--realtime", "--niter", "1"], ["--root", "r", "--out", "o", "--realtime", "--softmask"],
                 ["--root", "r", "--out", "o", "--window-seconds", "0"], ["--root", "r", "--out", "o", "--niter", "-1"]):
        with pytest.raises(SystemExit):
            E.parse_args(p, argv)
    # the flags the two command lines share are spelled alike
    from xumx_slicq_amd.inference import cli_parser
    theirs = {o for act in cli_parser()._actions for o in act.option_strings}
    assert {"--model-path", "--realtime", "--niter", "--softmask", "--device"} <= theirs & {o for act in p._actions for o in act.option_strings}


# ---- the JSON ------------------------------------------------------------------------------------------------------------
def _result(names, med, glo, frames):
    return {"metric": "framewise-sdr", "window": 1000, "silent": "any",
            "targets": {n: {"sdr_median": [m], "sdr_global": [g], "frames": np.asarray([frames])} for n, m, g in zip(names, med, glo)}}


def test_json_schema_and_aggregate():
    from xumx_slicq_amd.evaluation import aggregate_scores
    from xumx_slicq_amd.scoring import to_jsonable
    names = ("bass", "vocals", "other", "drums")
    nan, inf = float("nan"), float("inf")
    per_track = {"a": _result(names, [1.0, 2.0, nan, 4.0], [1.5, 2.5, -80.0, 4.5], [1.0, nan, inf, -inf]),
                 "b": _result(names, [3.0, 6.0, 7.0, 0.0], [3.5, 6.5, 7.5, 0.5], [0.0, 1.0, 2.0, 3.0]),
                 "c": _result(names, [2.0, 1.0, 9.0, 8.0], [2.5, 1.5, 9.5, 8.5], [0.0, 1.0, 2.0, 3.0])}
    agg = aggregate_scores(per_track)
    assert list(agg) == list(names) and set(agg["bass"]) == {"sdr_median", "sdr_global_mean", "sdr_global_median"}
    assert agg["bass"] == {"sdr_median": 2.0, "sdr_global_mean": 2.5, "sdr_global_median": 2.5}
    assert agg["other"]["sdr_median"] == 8.0 and agg["other"]["sdr_global_median"] == 7.5        # the all-silent track is left out of the median
    text = json.dumps(to_jsonable(per_track["a"]), allow_nan=False)                             # strict JSON: no NaN / Infinity tokens
    back = json.loads(text)
    assert back["metric"] == "framewise-sdr" and back["window"] == 1000 and back["silent"] == "any"
    assert back["targets"]["other"] == {"sdr_median": [None], "sdr_global": [-80.0], "frames": [[1.0, None, "inf", "-inf"]]}
    only_nan = aggregate_scores({"a": _result(names, [nan] * 4, [0.0] * 4, [nan])})
    assert np.isnan(only_nan["drums"]["sdr_median"])


# ---- symbols, and what stays --------------------------------------------------------------------------------------------
def test_score_symbols_are_declared_and_exported():
    from conftest import ROOT
    from xumx_slicq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    for name in ("xsq_score_workspace", "xsq_score_accumulate", "xsq_score_finalise", "xsq_score_max_frames"):
        assert name + "(" in hdr, name
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED, name
    assert "score.hip" in open(os.path.join(ROOT, "xumx_slicq_amd", "csrc", "Makefile")).read()
    assert _lib.lib.xsq_abi_version() == 2


def test_separate_and_evaluate_still_names_one_of_its_two_metrics():
    from xumx_slicq_amd.evaluation import evaluate_dataset, global_sdr, separate_and_evaluate          # noqa: F401

    import types
    from xumx_slicq_amd.separator import Separator
    rng = np.random.default_rng(3)
    stems = {n: rng.standard_normal((500, 2)).astype(np.float32) * 0.1 for n in Separator.sources}
    track = types.SimpleNamespace(audio=sum(stems.values()), rate=44100,
                                  targets={n: types.SimpleNamespace(audio=a) for n, a in stems.items()})

    class Oracle:
        sample_rate = torch.tensor(44100.0)
        to_dict = staticmethod(Separator.to_dict)

        def __call__(self, audio):
            return torch.stack([torch.from_numpy(stems[n].T.copy())[None] * 0.5 for n in Separator.sources])

    res = separate_and_evaluate(Oracle(), track, device="cpu")
    assert res["metric"] in ("museval-bsseval-v4", "global-sdr")
    if res["metric"] == "global-sdr":
        assert abs(res["scores"]["drums"] - global_sdr(stems["drums"], 0.5 * stems["drums"])) < 1e-4
