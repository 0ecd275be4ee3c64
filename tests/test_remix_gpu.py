"""Separator.remix / forward_aggregate / --remix on the MI355X: gain-weighted mixes of the stems through R inverse
transforms (xsq_separator_remix) against the stems of forward, the reference fixtures and the CLI's two loops."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
G3 = [[1, 0, 1, 1], [0, 1, 0, 0], [0.5, -1, 2, 0.25]]
RMS_TOL, MAX_TOL = 1e-4, 1e-3


@pytest.fixture(scope="module")
def seps():
    from xumx_slicq_amd.separator import seeded_separator
    return {
        "realtime": seeded_separator(realtime=True),
        "offline_phasemix": seeded_separator(realtime=False, wiener=False),
        "offline_wiener": seeded_separator(realtime=False),
    }


def _close_to_einsum(got, stems, G, rel_rms=2e-6, rel_max=2e-5):
    ref = torch.einsum("rt,tbcn->rbcn", torch.tensor(G, dtype=torch.float64), stems.double().cpu())
    d = got.double().cpu() - ref
    rms = float(d.pow(2).mean().sqrt()) / max(float(ref.pow(2).mean().sqrt()), 1e-30)
    mx = float(d.abs().max()) / max(float(ref.abs().max()), 1e-30)
    assert rms < rel_rms and mx < rel_max, (rms, mx)


@pytest.mark.parametrize("name", ["offline_phasemix", "offline_wiener", "realtime"])
def test_one_hot_gains_are_the_stems_bit_for_bit(seps, name):
    """Multiplying by one and adding zeros is exact, and every kernel works per row: R = 4 one-hot rows reproduce
    forward's four stems exactly -- stacked chunks plus a tail with nb = 2, and a batch split over several passes."""
    sep = seps[name]
    x = synth_audio(60000 * 3 + 12345, seed=91, nb_samples=2).cuda()
    x[1] *= 5.0
    try:
        sep.chunk_size = 60000
        for cap in (0, 10):                 # 10 item-slices per pass: every chunk's batch is split (shared Wiener maxima)
            sep.max_item_slices = cap
            stems = sep(x)
            mixes = sep.remix(x, torch.eye(4))
            assert mixes.shape == (4, 2, 2, x.shape[-1])
            for t in range(4):
                assert torch.equal(mixes[t], stems[t]), (name, cap, t)
            one = sep.remix(x, {"bass": 0, "other": 0, "drums": 0})       # R = 1: vocals only
            assert one.shape == (1, 2, 2, x.shape[-1]) and torch.equal(one[0], stems[1])
    finally:
        sep.chunk_size, sep.max_item_slices = 2621440, 0


@pytest.mark.parametrize("name", ["offline_phasemix", "offline_wiener"])
def test_general_gains_match_the_weighted_sum_of_the_stems(seps, name):
    sep = seps[name]
    x = synth_audio(60000 * 2 + 777, seed=92, nb_samples=2).cuda()
    try:
        sep.chunk_size = 60000
        stems = sep(x)
        got = sep.remix(x, G3)
        assert got.shape == (3, 2, 2, x.shape[-1]) and got.dtype == torch.float32
        _close_to_einsum(got, stems, G3)
        # the Python chunk loop (an A/B switch off its default) computes the same mixes by definition
        sep.native = False
        slow = sep.remix(x, G3)
    finally:
        sep.chunk_size = 2621440
        sep.native = True
    _close_to_einsum(slow, stems, G3)


@pytest.mark.parametrize("name", ["realtime", "offline_phasemix", "offline_wiener"])
def test_remix_matches_the_reference_stems(seps, name):
    g = load_golden("stems_9031.npz")
    sep = seps[name]
    n = 9031
    try:
        sep.chunk_size = int(g["chunk_size"])
        got = sep.remix(synth_audio(n, seed=20260101 + n).cuda(), G3).cpu()
    finally:
        sep.chunk_size = 2621440
    ref = torch.einsum("rt,tbcn->rbcn", torch.tensor(G3, dtype=torch.float64), torch.from_numpy(np.asarray(g[name])).double())
    d = got.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (name, rms, mx)


def test_forward_aggregate_matches_to_dict(seps):
    sep = seps["offline_wiener"]
    agg = {"vocals": ["vocals"], "accompaniment": ["bass", "drums", "other"]}
    x = synth_audio(60000 + 4321, seed=93).cuda()
    try:
        sep.chunk_size = 60000
        ref = sep.to_dict(sep(x), agg)
        got = sep.forward_aggregate(x, agg)
    finally:
        sep.chunk_size = 2621440
    assert list(got) == ["vocals", "accompaniment"]
    for k in got:
        assert got[k].shape == ref[k].shape == (1, 2, x.shape[-1])
    assert torch.equal(got["vocals"], ref["vocals"])
    _close_to_einsum(got["accompaniment"][None], ref["accompaniment"][None], [[1.0]])


@pytest.mark.parametrize("name", ["offline_phasemix", "offline_wiener"])
def test_remix_leaves_forward_and_the_input_alone(seps, name):
    sep = seps[name]
    x = synth_audio(60000 * 3 + 999, seed=94, nb_samples=2).cuda()
    x0 = x.clone()
    try:
        sep.chunk_size = 60000
        a = sep(x).clone()
        sep.remix(x, G3)
        sep.remix(x, [{"vocals": 0}])
        b = sep(x)
    finally:
        sep.chunk_size = 2621440
    assert torch.equal(a, b) and torch.equal(x, x0)
    with pytest.raises(ValueError):
        sep.remix(x.cpu(), G3)
    with pytest.raises(ValueError):
        sep.remix(x, {"voice": 0})


def test_cli_remix_pipelined_and_serial_write_the_same_files(tmp_path, seps):
    import subprocess
    import sys

    from conftest import ROOT
    from xumx_slicq_amd import audio as A
    (tmp_path / "in").mkdir()
    x = synth_audio(70001, seed=95)
    A.save_wav_float(str(tmp_path / "in" / "clip.wav"), x[0], 44100)
    for mode, extra in (("piped", []), ("serial", ["--serial"])):
        subprocess.run([sys.executable, "-m", "xumx_slicq_amd", "--input-dir", str(tmp_path / "in"), "--output-dir",
                        str(tmp_path / mode), "--remix", "karaoke:vocals=0"] + extra, check=True, cwd=ROOT, timeout=300)
        assert sorted(p.name for p in (tmp_path / mode / "clip").iterdir()) == ["karaoke.wav"]
    a = (tmp_path / "piped" / "clip" / "karaoke.wav").read_bytes()
    b = (tmp_path / "serial" / "clip" / "karaoke.wav").read_bytes()
    assert a == b and len(a) > 44
    # the CLI's default model: the offline stack with Wiener-EM
    sep = seps["offline_wiener"]
    stems = sep(x.cuda())
    y, rate = A.load_audio(str(tmp_path / "piped" / "clip" / "karaoke.wav"))
    assert rate == 44100 and y.shape == (2, 70001)
    _close_to_einsum(y[None, None], stems, [[1, 0, 1, 1]])
