"""Separator.remix without a GPU: the gain-matrix conversions (SPEC strings, dicts, lists, aggregate groups) and their
refusals, the C ABI's two remix entry points refusing bad arguments with an error code, and the combine kernel's
resources on gfx950."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_gain_rows_from_arrays_dicts_and_lists():
    from xumx_slicq_amd.separator import Separator, remix_gains
    assert Separator.sources == ["bass", "vocals", "other", "drums"]
    assert remix_gains([1, 0, 1, 1]).tolist() == [[1, 0, 1, 1]]
    assert remix_gains(torch.eye(4)).tolist() == torch.eye(4).tolist()
    import numpy as np
    assert remix_gains(np.full((2, 4), 0.5)).tolist() == [[0.5] * 4] * 2
    assert remix_gains({"vocals": 0}).tolist() == [[1, 0, 1, 1]]          # unnamed targets keep 1.0
    assert remix_gains({}).tolist() == [[1, 1, 1, 1]]
    G = remix_gains([{"vocals": 0}, {"bass": 0, "other": 0, "drums": 0}, {"drums": -2.5}])
    assert G.dtype == torch.float32 and G.shape == (3, 4)
    assert G.tolist() == [[1, 0, 1, 1], [0, 1, 0, 0], [1, 1, 1, -2.5]]


@pytest.mark.parametrize("bad", [
    {"voice": 0},                                   # unknown target
    [{"vocals": 0}, {"piano": 1}],
    [[1, 0, 0, 0]] * 5,                             # R > 4
    [{}] * 5,
    [],                                             # R = 0
    torch.zeros(0, 4),
    [1, 0, 0],                                      # not 4 targets
    torch.zeros(2, 2, 4),
    [1, float("nan"), 0, 0],                        # not finite
    {"drums": float("inf")},
    [[1, 0, 0, float("-inf")]],
    [{"vocals": 0}, [1, 0, 0, 0]],                  # mixed forms
    "vocals=0",
])
def test_gain_refusals(bad):
    from xumx_slicq_amd.separator import remix_gains
    with pytest.raises(ValueError):
        remix_gains(bad)


def test_aggregate_groups_are_zero_one_rows():
    from xumx_slicq_amd.separator import aggregate_gains
    names, G = aggregate_gains({"vocals": ["vocals"], "accompaniment": ["bass", "drums", "other"]})
    assert names == ["vocals", "accompaniment"]
    assert G.tolist() == [[0, 1, 0, 0], [1, 0, 1, 1]]
    names, G = aggregate_gains({"all": ["bass", "vocals", "other", "drums"], "bb": ["bass", "bass"]})
    assert G.tolist() == [[1, 1, 1, 1], [2, 0, 0, 0]]                       # named twice counts twice, as in to_dict
    for bad in ({}, {"a": ["bass"], "b": ["bass"], "c": ["bass"], "d": ["bass"], "e": ["bass"]}, {"x": ["guitar"]}, [["bass"]]):
        with pytest.raises(ValueError):
            aggregate_gains(bad)


def test_remix_spec_parser():
    from xumx_slicq_amd.inference import parse_remix_spec, parse_remix_specs
    assert parse_remix_spec("karaoke:vocals=0") == ("karaoke", [1.0, 0.0, 1.0, 1.0])
    assert parse_remix_spec("instrumental:vocals=0,drums=0.5") == ("instrumental", [1.0, 0.0, 1.0, 0.5])
    assert parse_remix_spec(" loud : bass = 2 , other=-1 ") == ("loud", [2.0, 1.0, -1.0, 1.0])
    assert parse_remix_spec("all:") == ("all", [1.0, 1.0, 1.0, 1.0])
    for bad in ("karaoke", ":vocals=0", "a/b:vocals=0", "..:vocals=0", "k:voice=0", "k:vocals", "k:vocals=x",
                "k:vocals=nan", "k:drums=inf", "k:vocals=0,vocals=1"):
        with pytest.raises(ValueError):
            parse_remix_spec(bad)
    assert parse_remix_specs(None) is None and parse_remix_specs([]) is None
    names, G = parse_remix_specs(["karaoke:vocals=0", "instrumental:vocals=0,drums=0.5"])
    assert names == ["karaoke", "instrumental"] and G.tolist() == [[1, 0, 1, 1], [1, 0, 1, 0.5]]
    with pytest.raises(ValueError):
        parse_remix_specs(["a:", "b:", "c:", "d:", "e:"])
    with pytest.raises(ValueError):
        parse_remix_specs(["a:vocals=0", "a:drums=0"])


def test_cli_refuses_a_bad_remix_before_any_work(capsys):
    from xumx_slicq_amd.inference import inference_main
    with pytest.raises(SystemExit) as e:
        inference_main(["--remix", "karaoke:voice=0", "--device", "cpu"])
    assert e.value.code == 2 and "voice" in capsys.readouterr().err


def test_library_exports_the_remix_entry_points():
    from xumx_slicq_amd import _lib
    for name in ("xsq_slicqt_inverse_remix", "xsq_slicqt_remix_workspace", "xsq_separator_remix"):
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED


def test_remix_entry_points_refuse_bad_arguments():
    """NULL pointers, R = 0, R = 5 and non-finite gains: an error code and a message, never a dereference (the gains and
    R are checked before any handle is touched, so a dummy host buffer stands in for the handles)."""
    from xumx_slicq_amd import _lib
    L = _lib.lib
    dummy = C.create_string_buffer(4096)
    h = C.addressof(dummy)
    ok = (C.c_float * 16)(*([1.0] * 16))
    nan = (C.c_float * 16)(*([1.0] * 5 + [math.nan] + [1.0] * 10))
    inf = (C.c_float * 16)(*([math.inf] + [1.0] * 15))

    def inv(plan, masks, mix, Y, gains, R, y=h, ws=h):
        return L.xsq_slicqt_inverse_remix(plan, masks, mix, Y, gains, R, 1, 4, 1000, y, None, ws, 4096, None)

    def sep(d, audio, gains, R, out=h):
        return L.xsq_separator_remix(d, h, audio, 1, 1000, 1000, 8, 0, 0, out, h, 4096, None, 0, None, None, gains, R)

    for rc_call, word in ((lambda: inv(None, None, None, h, ok, 1), "null"),
                          (lambda: inv(h, None, None, h, None, 1), "null"),
                          (lambda: inv(h, None, None, h, ok, 1, y=None), "null"),
                          (lambda: inv(h, None, None, h, ok, 0), "R=0"),
                          (lambda: inv(h, None, None, h, ok, 5), "R=5"),
                          (lambda: inv(h, None, None, h, nan, 2), "finite"),
                          (lambda: inv(h, None, None, h, inf, 1), "finite"),
                          (lambda: sep(None, h, ok, 1), "null"),
                          (lambda: sep(h, None, ok, 1), "null"),
                          (lambda: sep(h, h, None, 1), "null"),
                          (lambda: sep(h, h, ok, 0), "R=0"),
                          (lambda: sep(h, h, ok, 5), "R=5"),
                          (lambda: sep(h, h, nan, 2), "finite"),
                          (lambda: sep(h, h, inf, 1), "finite")):
        rc = rc_call()
        assert rc < 0, word
        assert word in _lib.last_error(), (word, _lib.last_error())
    assert L.xsq_slicqt_remix_workspace(None, 1, 1, 4, 0) == 0
    assert L.xsq_slicqt_remix_workspace(h, 0, 1, 4, 0) == 0 and L.xsq_slicqt_remix_workspace(h, 5, 1, 4, 0) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_remix_kernel_resources_on_gfx950(tmp_path):
    """The combine kernel, compiled as the product library compiles slicqt.hip: no scratch, no spills, well inside the
    register file, no packed-fp32 instruction."""
    csrc = os.path.join(ROOT, "xumx_slicq_amd", "csrc")
    asm = tmp_path / "slicqt.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "slicqt.hip"), "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=900, cwd=csrc)
    text = asm.read_text()
    meta = re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", text, flags=re.S)
    remix = [m for m in meta if "k_remix_combine" in m[0]]
    assert len(remix) == 1, meta
    name, scratch, vgprs = remix[0]
    assert int(scratch) == 0 and int(vgprs) <= 64, remix
    report = r.stderr.split("k_remix_combine", 1)[1].split("Function Name", 1)[0]
    assert re.search(r"VGPRs Spill: 0", report) and re.search(r"ScratchSize \[bytes/lane\]: 0", report), report
    body = text.split("k_remix_combine", 1)[1]
    body = body.split(".Lfunc_end", 1)[0]
    assert "global_load_dwordx4" in body or "buffer_load_dwordx4" in body       # one 16-byte load per target
    assert not re.search(r"v_pk_(fma|add|mul)_f32", text)
