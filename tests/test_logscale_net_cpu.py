"""The network on the logarithmic scales, host side: the ``long_bands`` / ``fgamma`` keywords from ``Separator.load``,
``load_target_models``, ``build_models`` and ``seeded_separator`` down to the plan, both command lines, the refusals that name the
keyword, and the fixture of the reference's own network (tests/golden/logscale_net*.npz, tools/make_golden_logscale_net.py).  Plans,
shapes and helpers are those of tests/test_logscale_cpu.py; owns the separators' configuration of tests/test_logscale_net_gpu.py.
"""
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import test_logscale_cpu as LC

SEED = 1234
NET_PLANS = ("A", "B")
MODELS = {"realtime": dict(realtime=True), "offline_phasemix": dict(realtime=False, wiener=False), "offline_wiener": dict(realtime=False)}
FIXTURE_MODELS = {"realtime": "realtime", "offline_wiener": "offline"}          # separator -> stems_<key>_<...> of the fixture
# (F, T) of the CDAE blocks: a band above 320 samples is a block of its own (F = 1, one frequency tap)
BLOCKS = {"A": [(3, 16), (1, 28), (1, 48), (1, 80), (1, 144), (1, 256), (1, 452), (1, 768), (1, 1020)],
          "B": 21, "D_longest": [(1, 8592), (1, 11240)]}


def net_config(key, **extra):
    scale, fbins, fmin, fgamma = LC.CONFIGS[key]
    return dict(fscale=scale, fbins=fbins, fmin=fmin, fgamma=fgamma, long_bands=True, seed=SEED, **extra)


def make_separator(key, model, device="cuda", **extra):
    from xumx_slicq_amd.separator import seeded_separator
    return seeded_separator(**MODELS[model], device=device, **net_config(key, **extra))


def block_shapes(key):
    return [(F, T) for (_, F, T) in LC.pkg_plan(key).blocks]


def make_sd(key):
    from xumx_slicq_amd.weights import seeded_state_dict
    return seeded_state_dict(block_shapes(key), seed=SEED)


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_logscale_net", os.path.join(ROOT, "tools", "make_golden_logscale_net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the keyword reaches the plan -----------------------------------------------------------------------------------------------------
def test_every_entry_point_has_the_two_keywords_with_their_defaults():
    from xumx_slicq_amd import separator as S
    for fn in (S.build_models, S.load_target_models, S.seeded_separator, S.Separator.load):
        p = inspect.signature(fn).parameters
        assert p["long_bands"].default is False and p["fgamma"].default == 15.0, fn
    assert isinstance(S.Separator.long_bands, property) and isinstance(S.Separator.dc_twins, property)


@pytest.mark.parametrize("key", ["A", "B"])
def test_the_keyword_reaches_the_plan_and_the_separator_reads_it_back(key):
    from xumx_slicq_amd.separator import build_models
    sep = make_separator(key, "realtime", device="cpu")
    plan = sep.nsgt.nsgt.plan
    assert sep.long_bands is True and plan.long_bands and not sep.dc_twins
    assert (plan.L, plan.Lg.tolist()) == LC.FACTS[key] and plan.fgamma == LC.CONFIGS[key][3] and plan.scale == LC.CONFIGS[key][0]
    assert [tuple(s) for s in sep.xumx_model.table.shapes] == block_shapes(key)
    if key == "A":
        assert block_shapes(key) == BLOCKS["A"]
        assert make_separator(key, "realtime", device="cpu", dc_twins=True).dc_twins
    else:
        assert len(block_shapes(key)) == BLOCKS["B"] and block_shapes(key)[-1] == (1, 2788) and (5, 16) in block_shapes(key)
        # fgamma moves the variable-Q plan: another offset is another plan
        scale, fbins, fmin, _ = LC.CONFIGS[key]
        _, (nsgt, _, _), _ = build_models(scale, fbins, fmin, device="cpu", long_bands=True, fgamma=0.0)
        assert nsgt.nsgt.plan.fgamma == 0.0 and nsgt.nsgt.plan.Lg.tolist() != LC.FACTS[key][1]
    bark = make_separator_bark()
    assert bark.long_bands is False


def make_separator_bark():
    from xumx_slicq_amd.separator import seeded_separator
    return seeded_separator(realtime=True, device="cpu")


def test_plan_d_has_the_two_blocks_of_the_8192_point_class():
    assert block_shapes("D")[-2:] == BLOCKS["D_longest"]


# ---- 2. without the keyword: today's refusal ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["cqlog", "vqlog"])
def test_without_the_keyword_the_two_scales_are_refused_with_todays_text(scale):
    from xumx_slicq_amd.plan import build_plan
    from xumx_slicq_amd.separator import build_models, seeded_separator
    with pytest.raises(ValueError) as want:
        build_plan(scale, 10, 130.0)
    assert "long_bands=True" in str(want.value)
    for call in (lambda: build_models(scale, 10, 130.0, device="cpu"), lambda: seeded_separator(fscale=scale, fbins=10, fmin=130.0, device="cpu"),
                 lambda: build_models(scale, 10, 130.0, device="cpu", long_bands=False, fgamma=3.0)):
        with pytest.raises(ValueError) as got:
            call()
        assert str(got.value) == str(want.value)


# ---- 3. the state dict has the reference's names and shapes -----------------------------------------------------------------------------
@pytest.mark.parametrize("key", NET_PLANS)
def test_state_dict_has_the_names_and_shapes_the_reference_recorded(key):
    g = load_golden("logscale_net.npz")
    names, shapes = [str(s) for s in g[f"sd_names_{key}"]], g[f"sd_shapes_{key}"]
    for model in ("realtime", "offline_wiener"):
        sd = make_separator(key, model, device="cpu").xumx_model.state_dict()
        assert list(sd) == names
        for k, row in zip(names, shapes):
            assert tuple(sd[k].shape) == tuple(int(v) for v in row[:sd[k].dim()]) and not row[sd[k].dim():].any(), k
    seeded = make_sd(key)
    assert set(seeded) == set(names) and all(tuple(seeded[k].shape) == tuple(int(v) for v in row[:seeded[k].dim()]) for k, row in zip(names, shapes))
    assert int(g["seed"]) == SEED and int(g[f"n_{key}"]) == LC.lengths(LC.pkg_plan(key))[1]
    for fx in FIXTURE_MODELS.values():
        st = g[f"stems_{key}_{fx}"]
        assert st.shape == (4, 1, 2, int(g[f"n_{key}"])) and st.dtype == np.float32 and np.isfinite(st).all() and float(np.abs(st).max()) > 1e-3


def test_the_fixture_tool_feeds_the_input_of_the_logscale_tests():
    tool = _tool()
    assert tool.SEED == SEED and tool.PLANS == {k: LC.CONFIGS[k] for k in NET_PLANS}
    assert torch.equal(tool.audio(4232, 2), LC.audio(4232, 2))


# ---- 4. load_target_models: fgamma from the JSON ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_json", [True, False])
def test_load_target_models_passes_fgamma_from_the_json(tmp_path, monkeypatch, in_json):
    from xumx_slicq_amd import separator as S
    args = {"fscale": "vqlog", "fbins": 24, "fmin": 40.0, "sample_rate": 44100.0, "seq_dur": 2.0, "realtime": True}
    if in_json:
        args["fgamma"] = 7.5
    (tmp_path / "xumx_slicq_v2.json").write_text(json.dumps({"args": args}))
    torch.save({"w": torch.zeros(4096)}, tmp_path / "xumx_slicq_v2.pth")
    seen = {}

    def fake(*a, **kw):
        seen["a"], seen["kw"] = a, kw
        return "model", ("nsgt", "insgt", "cnorm"), 44100.0

    monkeypatch.setattr(S, "build_models", fake)
    S.load_target_models(str(tmp_path), long_bands=True, fgamma=3.0)
    assert seen["a"][:3] == ("vqlog", 24, 40.0) and seen["kw"]["long_bands"] is True and seen["kw"]["dc_twins"] is False
    assert seen["kw"]["fgamma"] == (7.5 if in_json else 3.0)
    S.load_target_models(str(tmp_path))
    assert seen["kw"]["long_bands"] is False and seen["kw"]["fgamma"] == (7.5 if in_json else 15.0)


# ---- 5. both command lines ----------------------------------------------------------------------------------------------------------------
def test_both_command_lines_parse_the_new_flags(capsys):
    from xumx_slicq_amd import evaluation, inference
    a = inference.parse_args(inference.cli_parser(), [])
    assert a.long_bands is False and a.fgamma == 15.0
    a = inference.parse_args(inference.cli_parser(), ["--model-path", "M", "--long-bands", "--fgamma", "20"])
    assert a.long_bands is True and a.fgamma == 20.0
    with pytest.raises(SystemExit):
        inference.parse_args(inference.cli_parser(), ["--long-bands", "--realtime", "--stream", "4096"])
    assert "--long-bands" in capsys.readouterr().err
    e = evaluation.parse_args(evaluation.cli_parser(), ["--root", "D", "--out", "O"])
    assert e.long_bands is False and e.fgamma == 15.0
    e = evaluation.parse_args(evaluation.cli_parser(), ["--root", "D", "--out", "O", "--long-bands", "--fgamma", "0"])
    assert e.long_bands is True and e.fgamma == 0.0


# ---- 6. the four refusals name the keyword ------------------------------------------------------------------------------------------------
def test_stream_trainer_demix_into_and_sharding_refuse_naming_long_bands():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.sharding import ShardedDemixer
    from xumx_slicq_amd.training import Trainer
    sep = make_separator("A", "realtime", device="cpu")
    n = LC.lengths(LC.pkg_plan("A"))[0]
    with pytest.raises(_lib.XsqError, match="long_bands"):
        sep.stream()
    with pytest.raises(_lib.XsqError, match="long_bands"):
        Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), precision="fp32")
    with pytest.raises(_lib.XsqError, match="long_bands"):
        sep.demix_into(LC.audio(n, 2)[None], torch.empty(4, 1, 2, n), torch.zeros(4, 1, 2, dtype=torch.int64))
    with pytest.raises(_lib.XsqError, match="long_bands"):
        ShardedDemixer(sep, [n], lambda item: None, torch.device("cpu"))
