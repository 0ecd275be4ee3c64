"""Host side of xumx_slicq_amd/slicqfinder.py: the draw table, the command line, the reroll bookkeeping of the search, the
fixture's own consistency, and the argument checks of the three new entry points (no device needed: they run before any HIP
call)."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

_spec = importlib.util.spec_from_file_location("make_golden_ideal", os.path.join(ROOT, "tools", "make_golden_ideal.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

NEW_SYMBOLS = ("xsq_wiener_sources_workspace", "xsq_wiener_em_sources", "xsq_phasemix_sources", "xsq_ideal_workspace", "xsq_ideal_separate")


def test_draw_table_is_a_pure_function_of_the_seed_and_stays_in_range():
    from xumx_slicq_amd.slicqfinder import draw_params
    args = (["bark", "mel"], (10, 300), (10, 130, 0.1))
    a, b = draw_params(42, 200, *args), draw_params(42, 200, *args)
    assert a == b and len(a) == 200
    assert a != draw_params(43, 200, *args)
    np.random.seed(1)
    assert draw_params(42, 200, *args) == a                      # the global generators play no part
    assert {s for s, _, _ in a} == {"bark", "mel"}
    assert all(10 <= bins < 300 and isinstance(bins, int) for _, bins, _ in a)
    grid = np.arange(10, 130, 0.1)
    assert all(10 <= f < 130 and np.abs(grid - f).min() == 0 for _, _, f in a)
    with pytest.raises(ValueError):
        draw_params(1, 3, [], (10, 300), (10, 130, 0.1))
    with pytest.raises(ValueError):
        draw_params(1, 3, ["mel"], (10, 10), (10, 130, 0.1))


def test_cli_defaults_and_parsing():
    from xumx_slicq_amd.slicqfinder import DEFAULT_PIECE, cli_parser, parse_args
    a = parse_args(cli_parser(), ["--root", "D"])
    assert (a.fbins, a.fmins, a.n_iter, a.fscale, a.oracle_strategy, a.random_seed, a.max_sllen, a.single, a.per_target) == \
        ("10,300", "10,130,0.1", 60, "bark,mel", "wiener", 42, 44100, False, False)
    assert a.params == {"scales": ["bark", "mel"], "bins": (10, 300), "fmin": (10.0, 130.0, 0.1)}
    assert (a.valid, a.storage, a.piece, a.out) == (None, "fp32", DEFAULT_PIECE, "slicqfinder.json") and DEFAULT_PIECE == 2621440
    a = parse_args(cli_parser(), ["--root", "D", "--valid", "A,B", "--n-iter", "3", "--per-target", "--oracle-strategy", "phasemix",
                                  "--fscale", "mel", "--fbins", "20,40", "--fmins", "100,120,0.5", "--random-seed", "7", "--piece", "44100"])
    assert a.valid == ["A", "B"] and a.n_iter == 3 and a.per_target and a.oracle_strategy == "phasemix" and a.piece == 44100
    assert a.params == {"scales": ["mel"], "bins": (20, 40), "fmin": (100.0, 120.0, 0.5)} and a.random_seed == 7
    a = parse_args(cli_parser(), ["--root", "D", "--single", "--fscale", "bark", "--fbins", "262", "--fmins", "32.9"])
    assert a.single and a.params == {"scale": "bark", "bins": 262, "fmin": 32.9}
    for bad in (["--fscale", "cqlog"], ["--fscale", "bark,cqlog"], ["--fscale", "octave"], ["--fbins", "10"], ["--fmins", "10,130"],
                ["--n-iter", "0"], ["--single"], ["--oracle-strategy", "softmask"]):
        with pytest.raises(SystemExit):
            parse_args(cli_parser(), ["--root", "D"] + bad)


def test_cqlog_is_refused_by_name(capsys):
    from xumx_slicq_amd.slicqfinder import cli_parser, parse_args
    with pytest.raises(SystemExit):
        parse_args(cli_parser(), ["--root", "D", "--fscale", "cqlog"])
    assert "cqlog" in capsys.readouterr().err


class StubOracle:
    """Scores a draw by its bin count; every draw with an odd bin count is refused with four -inf."""

    def __init__(self):
        self.calls, self.refusals = [], []

    def oracle(self, scale, fmin, bins):
        self.calls.append((scale, bins, fmin))
        if bins % 2:
            self.refusals.append({"scale": scale, "bins": bins, "fmin": fmin, "reason": "odd"})
            return (float("-inf"),) * 4
        return (bins / 10.0, -bins / 10.0, fmin, 1.0)


@pytest.mark.parametrize("per_target", [False, True])
def test_optimize_many_rerolls_refusals_and_keeps_the_best(per_target, tmp_path):
    from xumx_slicq_amd.slicqfinder import draw_params, optimize_many
    params = {"scales": ["bark", "mel"], "bins": (10, 300), "fmin": (10, 130, 0.1)}
    stub = StubOracle()
    out = str(tmp_path / "r.json")
    res = optimize_many(stub.oracle, params, 5, per_target, seed=3, out=out, refusals=stub.refusals)
    table = draw_params(3, 8 * 5 + 8, params["scales"], params["bins"], params["fmin"])
    assert stub.calls == table[:len(stub.calls)]                  # the draws are the table's rows, in order
    scored = [c for c in stub.calls if c[1] % 2 == 0]
    assert len(scored) == 5 == len(res["rounds"]) and stub.calls[-1] == scored[-1]
    assert res["rerolled"] == len(stub.calls) - 5 == len(res["refusals"]) and res["rerolled"] > 0
    assert [(r["scale"], r["bins"], r["fmin"]) for r in res["refusals"]] == [c for c in stub.calls if c[1] % 2]
    assert all(r["reason"] == "odd" for r in res["refusals"]) and not res["exhausted"]
    if per_target:
        assert res["best"]["bass"]["params"] == max(scored, key=lambda c: c[1])
        assert res["best"]["drums"]["params"] == min(scored, key=lambda c: c[1])
        assert res["best"]["vocals"]["sdr"] == max(c[2] for c in scored) and res["best"]["other"]["sdr"] == 1.0
    else:
        tot = [(c[1] / 10.0 - c[1] / 10.0 + c[2] + 1.0) / 4 for c in scored]
        assert res["best"]["total"]["sdr"] == max(tot) and tuple(res["best"]["total"]["params"]) == scored[int(np.argmax(tot))]
    assert json.load(open(out))["rerolled"] == res["rerolled"]


def test_a_search_that_finds_nothing_says_so():
    from xumx_slicq_amd.slicqfinder import NO_REASON, evaluate_single, optimize_many
    res = optimize_many(lambda **kw: (float("-inf"),) * 4, {"scales": ["mel"], "bins": (10, 20), "fmin": (10, 20, 1)}, 2, seed=0)
    assert res["exhausted"] and res["rounds"] == [] and res["rerolled"] == 8 * 2 + 8 and res["best"]["total"]["params"] is None
    # an oracle that gives no reason (a closure, no list handed over): every refused draw is still named, and says so
    assert len(res["refusals"]) == 8 * 2 + 8 and all(r["reason"] == NO_REASON for r in res["refusals"])
    single = evaluate_single(lambda **kw: (float("-inf"),) * 4, {"scale": "mel", "bins": 12, "fmin": 11.0})
    assert single["refusals"] == [{"scale": "mel", "bins": 12, "fmin": 11.0, "reason": NO_REASON}]
    assert evaluate_single(lambda **kw: (1.0, 2.0, 3.0, 4.0), {"scale": "mel", "bins": 12, "fmin": 11.0})["refusals"] == []


def test_fixture_sdrs_are_the_global_sdr_of_its_own_estimates():
    from xumx_slicq_amd.evaluation import global_sdr
    g = load_golden("ideal_oracle.npz")
    for key in G.CASES:
        src = G.case_sources(key)
        for j in range(4):
            est = g[f"est_{key}_{j}"]
            assert est.shape == src[j].shape and est.dtype == np.float32
            assert abs(global_sdr(src[j].T, est.T) - g[f"sdr_{key}"][j]) < 1e-3, (key, j)
    assert not g["est_mz1_2"].any() and g["sdr_mz1"][2] == 0.0
    assert not any(g[f"est_mz4_{j}"].any() for j in range(4)) and not g["sdr_mz4"].any()


def test_new_symbols_are_exported_and_declared():
    from xumx_slicq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xumx_slicq_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTED and n + "(" in hdr, n


def test_null_and_bad_arguments_are_rejected_not_crashed():
    from xumx_slicq_amd import _lib
    L = _lib.lib
    F, T = np.asarray([2, 1], dtype=np.int32), np.asarray([8, 12], dtype=np.int32)
    geo = (2, F.ctypes.data, T.ctypes.data)
    buf = np.zeros(96, dtype=np.float32)            # never read: every call below fails its checks first
    p = (buf.ctypes.data + 63) // 64 * 64
    assert L.xsq_wiener_em_sources(0, None, None, None, None, 1, 3, 5000, 1, None, 0, None) == -1
    assert L.xsq_wiener_em_sources(*geo, None, p, 1, 3, 5000, 1, p, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.xsq_wiener_em_sources(*geo, p, None, 1, 3, 5000, 1, p, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.xsq_wiener_em_sources(*geo, p, p, 1, 3, 5000, 1, None, 1 << 20, None) == -1 and "null" in _lib.last_error()
    assert L.xsq_wiener_em_sources(*geo, p, p, 0, 3, 5000, 1, p, 1 << 20, None) == -1
    assert L.xsq_wiener_em_sources(*geo, p, p, 1, 3, -5, 1, p, 1 << 20, None) == -1 and "win_len" in _lib.last_error()
    assert L.xsq_wiener_em_sources(*geo, p, p, 2, 3, 5000, 3, p, 1 << 20, None) == -1 and "batch_group" in _lib.last_error()
    assert L.xsq_wiener_em_sources(*geo, p, p, 1, 3, 5000, 1, p, 16, None) == -1 and "workspace too small" in _lib.last_error()
    assert L.xsq_wiener_em_sources(*geo, p + 4, p, 1, 3, 5000, 1, p, 1 << 20, None) == -1 and "aligned" in _lib.last_error()
    assert L.xsq_wiener_sources_workspace(0, None, None, 1, 3, 5000) == 0
    assert L.xsq_wiener_sources_workspace(*geo, 1, 3, 5000) == L.xsq_wiener_workspace(*geo, 1, 3, 5000) > 0
    assert L.xsq_wiener_sources_workspace(*geo, 1, 3, 0) == L.xsq_wiener_workspace(*geo, 1, 3, 36)          # one window per row
    # rows longer than the default 5000 frames: 0 is ONE window per row (6000 and 24 frames), not the default's two and one
    Tl = np.asarray([2000, 8], dtype=np.int32)
    gl = (2, F.ctypes.data, Tl.ctypes.data)
    one, dflt = L.xsq_wiener_sources_workspace(*gl, 1, 3, 0), L.xsq_wiener_sources_workspace(*gl, 1, 3, 5000)
    assert one == L.xsq_wiener_workspace(*gl, 1, 3, 6000) and dflt == L.xsq_wiener_workspace(*gl, 1, 3, 5000)
    assert dflt - one == 2 * 24 * 4                  # the two rows of block 0 have one 24-float slot fewer each
    assert L.xsq_phasemix_sources(0, None, None, None, None, 1, 3, None) == -1
    assert L.xsq_phasemix_sources(*geo, None, p, 1, 3, None) == -1 and "null" in _lib.last_error()
    assert L.xsq_phasemix_sources(*geo, p, p, 1, 0, None) == -1
    assert L.xsq_phasemix_sources(*geo, p, p + 4, 1, 3, None) == -1 and "aligned" in _lib.last_error()
    assert L.xsq_ideal_workspace(None, 1, 9031, 0, 5000) == 0 and "null" in _lib.last_error()
    assert L.xsq_ideal_separate(None, p, 1, 9031, 0, 5000, p, p, 1 << 20, None) == -1 and "null" in _lib.last_error()


def test_cpu_tensors_and_misshapen_sources_are_refused_loudly():
    import torch
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    from xumx_slicq_amd.transforms import NSGTBase
    base = NSGTBase("mel", 32, 115.5, device="cpu")
    with pytest.raises(_lib.XsqError, match="ROCm device only"):
        ideal_slicqt(torch.zeros(4, 1, 2, 9031), base)
    with pytest.raises(ValueError, match="four sources"):
        ideal_slicqt(torch.zeros(3, 1, 2, 9031), base)
    with pytest.raises(_lib.XsqError, match="one EM iteration"):
        ideal_slicqt(torch.zeros(4, 1, 2, 9031), base, niter=0)
    with pytest.raises(ValueError):
        ideal_slicqt(torch.zeros(4, 1, 2, 9031), base, strategy="ratio")
