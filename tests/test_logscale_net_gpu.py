"""The network on the logarithmic scales, on the device: ``Separator`` with ``long_bands=True`` on plans whose bands above Lg 320 run
on the FFT band engine (csrc/band_fft.h) -- the whitened magnitude that engine's analysis writes for the CDAE, the CDAE and the
Wiener-EM filter on blocks of F = 1 and thousands of frames, and every entry point that serves such a plan.
tests/test_logscale_cpu.py owns the plans (A = ``cqlog, 10, 130.0``: long blocks of T 452, 768, 1020; B = ``vqlog, 24, 40.0``: nine
long blocks up to T 2788 and a five-band block of T 16; D = ``cqlog, 15, 12.0``: blocks of T 8592 and 11240 on the 8192-point FFT class),
the shapes (n = 2 h + 1: S = 3, and n = 7 h + 123: S = 5 with a ragged tail) and the helpers; tests/test_logscale_net_cpu.py the
separators' configuration.

Float64 parity follows tests/test_ref64_plans_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err``, E the LARGEST fp32-oracle error over the
members of the stage on the same input, M per stage the smallest power of two at least twice the worst e_gpu / E measured on MI355X
(profiles/logscale_net_parity.json), at most ``M_CAP``.  S = 3 runs with nb_samples 2 and S = 5 with nb_samples 1.  The float64
comparisons run on the default engine (``dc_twins=False``: the 0.007 share of A is dropped by contract, as ``ref64.inverse`` drops
it); the reference's fixture (tests/golden/logscale_net*.npz) is met with ``dc_twins=True`` on A.

Wall time of the module on MI355X: 18 s for its 49 tests in one process (the slowest, the epilogue's bits on A and B and the
Separator's on B realtime, 2.0 .. 2.2 s each with their first plans and models; everything else below 1 s).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import model as omodel
from oracle import ref64
from oracle import separator as osep
from oracle.parity import M_CAP, Tables
from test_logscale_cpu import audio, lengths, oracle_plan, pkg_plan
from test_logscale_net_cpu import FIXTURE_MODELS, MODELS, NET_PLANS, block_shapes, make_sd, make_separator
from test_ref64_gpu import _mask_errors
from test_ref64_mel_cpu import one_thread, windows
from test_wiener_options_cpu import wiener_options

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3             # the contractual bar

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/logscale_net_parity.json)
M = {
    "cdae": 4,                     # 1.30  (D, S = 3, B = 2, realtime: block 12, F 1, T 8592; A 1.04 at T 768, B 1.20 at its five-band block of T 16)
    "wiener": 4,                   # 1.08  (B, S = 3, B = 2, blockwise_wiener: block 20, T 2788, two windows; the masked form 1.04)
    "stems": 4,                    # 1.41  (A, realtime, n 1175, B = 2, stem 2; B at most 1.14)
    "wiener_options": 2,           # 0.83  (A, S = 5, B = 2, softmask + residual: block 1, T 28)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("logscale_net_parity", M)
_judge = _T.judge
SHAPES = [(0, 2), (1, 1)]                 # (index into lengths(plan), nb_samples): S = 3 with two items, S = 5 with one
CAUSAL = {"realtime": True, "offline_phasemix": False, "offline_wiener": False}
_SEPS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


def _sep(key, model, dc_twins=False):
    if (key, model, dc_twins) not in _SEPS:
        _SEPS[key, model, dc_twins] = make_separator(key, model, dc_twins=dc_twins)
    return _SEPS[key, model, dc_twins]


@pytest.fixture(scope="module", autouse=True)
def _drop_separators():
    yield
    for s in _SEPS.values():
        s.drop_graphs()
    _SEPS.clear()


def _input(key, idx, nb):
    n = lengths(pkg_plan(key))[idx]
    return audio(n, 2 * nb).view(nb, 2, n)


def _labels(key, S=None):
    return [f"block {b} F {F} T {T}" + ("" if S is None else f" windows {windows(S, T)[0]}") for b, (F, T) in enumerate(block_shapes(key))]


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the epilogue of the FFT band engine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["A", "B", "D"])
def test_whitened_magnitude_of_the_fft_band_engine_has_the_bits_of_the_magnitude_pass(key):
    """``eng.forward(x, whiten=...)`` leaves the coefficient arena of ``eng.forward(x)`` bit for bit, and its ``xin`` arena holds the
    bits the model's own magnitude pass (k_magnitude_whiten) writes from that arena -- in fp32 and in the split-bf16 operand format;
    S = 3 with two items and (A, B) S = 5 with one.  The arena is poisoned first: every word must have been written."""
    sep = _sep(key, "offline_phasemix")
    eng, m = sep.nsgt.nsgt.nsgt, sep.xumx_model
    assert sep.long_bands and max(T for _, T in block_shapes(key)) > 320
    try:
        for idx, nb in SHAPES[:1 if key == "D" else 2]:
            x = _input(key, idx, nb).cuda()
            for precision in ("fp32", "bf16x3"):
                m.set_precision(precision)
                plain, lead, S = eng.forward(x)
                ws, mean, scale, split = m.whitening_target(x.device, nb, S)
                assert split == (precision == "bf16x3") and lead == (nb, 2) and S == (3, 5)[idx]
                words = ws.view(torch.int32)[:plain.numel() // 2]
                words.fill_(0x7fc00001)
                fused, _, _ = eng.forward(x, whiten=(ws.data_ptr(), mean, scale, split))
                got = words.clone()
                assert torch.equal(_bits(fused), _bits(plain)), (key, idx, precision)
                m(eng.table.views(plain, lead, S))                         # xin_ready False: the magnitude pass writes the same workspace
                want = words.clone()
                assert not bool((got == 0x7fc00001).any()) and torch.equal(got, want), (key, idx, precision, int((got != want).sum()))
    finally:
        m.set_precision("fp32")


# ---- 2. the bits through the Separator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("key", NET_PLANS)
def test_whitening_fused_into_the_analysis_epilogues_is_bitwise_equal(key, model):
    """test_model_gpu.py's test of the same name on A and B: ``fuse_whiten = False`` (the Python chunk loop with the model's own
    magnitude pass) against the default, nb_samples 2 at S = 5, fp32 and bf16x3."""
    sep = _sep(key, model)
    x = _input(key, 1, 2).cuda()
    try:
        for precision in ("fp32", "bf16x3"):
            sep.xumx_model.set_precision(precision)
            sep.fuse_whiten = False
            a = sep(x).clone()
            sep.fuse_whiten = True
            b = sep(x).clone()
            assert a.shape == (4, 2, 2, x.shape[-1]) and bool(torch.isfinite(a).all())
            assert torch.equal(a, b), (key, model, precision, float((a - b).abs().max()))
    finally:
        sep.fuse_whiten = True
        sep.xumx_model.set_precision("fp32")


# ---- 3. float64 parity -------------------------------------------------------------------------------------------------------------------
def _cdae_case(key, idx, nb, model, blocks=None):
    """(failures, worst ratio) of the masks of ``blocks`` (default: all) against ref64.cdae_masks on the GPU's own coefficients."""
    sd, causal = make_sd(key), CAUSAL[model]
    sep = _sep(key, model)
    X = sep.nsgt(_input(key, idx, nb).cuda())
    _, masks = sep.xumx_model(X, return_masks=True)
    blocks = list(range(len(X))) if blocks is None else blocks
    Xc = [X[b].cpu() for b in blocks]
    ref = [ref64.cdae_masks(sd, b, ref64.abs_of_real_complex(Xb), causal) for b, Xb in zip(blocks, Xc)]
    with one_thread():
        e_cpu = _mask_errors([omodel.cdae_masks(sd, b, omodel.abs_of_real_complex(Xb), causal) for b, Xb in zip(blocks, Xc)], ref)
    got = [masks[b].cpu() for b in blocks]
    assert all(g.shape == r.shape and bool(torch.isfinite(g).all()) for g, r in zip(got, ref))
    labels = [_labels(key)[b] for b in blocks]
    return _judge("cdae", f"{key} S={(3, 5)[idx]} B={nb} {model}", _mask_errors(got, ref), e_cpu, labels, full_table=True)


@pytest.mark.parametrize("model", ["realtime", "offline_phasemix"])
@pytest.mark.parametrize("idx,nb", SHAPES)
@pytest.mark.parametrize("key", NET_PLANS)
def test_cdae_masks_of_every_block_are_at_fp32_rounding_of_float64(key, idx, nb, model):
    """Every block of A and B, the causal and the offline first layer: the long blocks are F = 1, one frequency tap, a layer-1 K of
    2 T and T layer-4 columns.  (The offline Wiener model's CDAE is the offline mix-phase model's: same weights, same launches.)"""
    bad, _ = _cdae_case(key, idx, nb, model)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("model", ["realtime", "offline_phasemix"])
def test_cdae_masks_of_the_two_longest_blocks_of_d_are_at_fp32_rounding_of_float64(model):
    """T 8592 and 11240 at S = 3: layer-1 rows of 2 T = 22480 products, layer 4 with 11240 columns."""
    nb = len(block_shapes("D"))
    assert [block_shapes("D")[b][1] for b in (nb - 2, nb - 1)] == [8592, 11240]
    bad, _ = _cdae_case("D", 0, 2, model, blocks=[nb - 2, nb - 1])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("idx,nb", SHAPES)
@pytest.mark.parametrize("key", NET_PLANS)
def test_wiener_em_of_every_block_is_at_fp32_rounding_of_float64(key, idx, nb):
    """The masked form the separator runs (Unmix.forward) and the module-level ``blockwise_wiener`` against ref64.blockwise_wiener;
    with two items, item 1 is forty times louder (the window maximum is shared over the batch).  Rows of 3 T .. 5 T frames: shorter
    than one 5000-frame window on most blocks, several windows on B's longest (5 x 2788), a window shorter than a slice nowhere
    on A and B (D's blocks: the CDAE test above)."""
    from xumx_slicq_amd.phase import blockwise_wiener
    sep = _sep(key, "offline_wiener")
    x = _input(key, idx, nb)
    x[nb - 1] *= 40.0 if nb > 1 else 1.0
    X = sep.nsgt(x.cuda())
    S = X[0].shape[3]
    Y, masks = sep.xumx_model(X, return_masks=True)
    g_masked, g_module, c = [], [], []
    for b in range(len(X)):
        Xb, mb = X[b].cpu(), masks[b].cpu()
        ref = ref64.blockwise_wiener(Xb, mb.double() * ref64.abs_of_real_complex(Xb))
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        ref_m = ref64.blockwise_wiener(Xb, Ymag)
        c.append(ref64.rel_err(omodel.blockwise_wiener(Xb, Ymag), ref_m))
        g_masked.append(ref64.rel_err(Y[b], ref))
        g_module.append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda()), ref_m))
    bad = []
    for tag, g in (("masked (Unmix.forward)", g_masked), ("blockwise_wiener", g_module)):
        b, _ = _judge("wiener", f"{key} S={S} B={nb} {tag}", _pair(g), _pair(c), _labels(key, S), full_table=True)
        bad += [f"{tag} {m}" for m in b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("idx,nb", SHAPES)
@pytest.mark.parametrize("key", NET_PLANS)
def test_stems_are_at_fp32_rounding_of_float64(key, idx, nb, model):
    """Separator.forward against ref64.separate over ``oracle_plan(key)``, per stem; the contractual bar beside the tight one."""
    plan, sd = oracle_plan(key), make_sd(key)
    causal, wiener = CAUSAL[model], model == "offline_wiener"
    x = _input(key, idx, nb)
    n = x.shape[-1]
    est = _sep(key, model)(x.cuda()).cpu()
    ref = ref64.separate(plan, sd, x, causal=causal, wiener=wiener)
    with one_thread():
        orc = osep.separate(plan, sd, x, causal=causal, wiener=wiener)
    assert est.shape == ref.shape == (4, nb, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (key, model, n, rms, mx)
    bad, _ = _judge("stems", f"{key} {model} n={n} B={nb}", ref64.rel_err(est, ref, keep=(0,)), ref64.rel_err(orc, ref, keep=(0,)),
                    [f"stem {t}" for t in range(4)], full_table=True)
    assert not bad, "\n".join(bad)


# ---- 4. the reference's own network ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(FIXTURE_MODELS))
@pytest.mark.parametrize("key", NET_PLANS)
def test_stems_equal_the_reference_fixture(key, model):
    """The reference's ``Separator.forward`` with the same seeded weights (tests/golden/logscale_net*.npz), n = 7 h + 123: realtime
    and offline (Wiener-EM); A with ``dc_twins=True``, since the reference computes the mirrored term."""
    g = load_golden("logscale_net.npz")
    n = int(g[f"n_{key}"])
    sep = _sep(key, model, dc_twins=(key == "A"))
    assert sep.dc_twins == (key == "A") and sep.long_bands
    est = sep(audio(n, 2)[None].cuda()).cpu()
    d = est.double() - torch.from_numpy(g[f"stems_{key}_{FIXTURE_MODELS[model]}"]).double()
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    print(f"[fixture] {key} {model}: stems against the reference's: rms {rms:.2e} max {mx:.2e}")
    _T.record("fixture", f"{key} {model}", {"M_key": "fixture (absolute distance from the reference's stems; bar 1e-4 RMS / 1e-3 max)",
                                            "worst_ratio": max(rms / RMS_TOL, mx / MAX_TOL), "rms": rms, "max": mx})
    assert rms < RMS_TOL and mx < MAX_TOL, (key, model, rms, mx)


# ---- 5. every served entry point, on A ---------------------------------------------------------------------------------------------------
def test_forward_graphed_is_bitwise_eager_and_a_second_forward_gives_the_same_bits():
    for model in MODELS:
        sep = _sep("A", model)
        x = _input("A", 1, 2).cuda()
        a = sep(x).clone()
        assert torch.equal(a, sep(x)), model
        assert torch.equal(a, sep.forward_graphed(x)) and torch.equal(a, sep.forward_graphed(x)), model


@pytest.mark.parametrize("model", ["realtime", "offline_wiener"])
def test_forward_overlapped_is_forward_of_each_segment_outside_the_fades(model):
    from xumx_slicq_amd.separator import segment_lengths, segments
    sep = _sep("A", model)
    segment, overlap = 0.1, 0.01
    chunk_len, ov = segment_lengths(float(sep.sample_rate), segment, overlap, sep.chunk_size)
    assert (chunk_len, ov) == (4454, 441)
    N = 2 * chunk_len + 500
    x = audio(N, 2)[None].cuda()
    out = sep.forward_overlapped(x, segment, overlap)
    segs = segments(N, chunk_len, ov)
    assert out.shape == (4, 1, 2, N) and len(segs) == 3
    for start, n, fade_in, fade_out in segs:
        own = sep(x[..., start:start + n].contiguous())
        assert torch.equal(out[..., start + fade_in:start + n - fade_out], own[..., fade_in:n - fade_out]), (model, start)


@pytest.mark.parametrize("model", ["realtime", "offline_wiener"])
def test_remix_matches_forward_and_the_gain_sum(model):
    """``{"vocals": 0}`` (karaoke) against einsum of the stems, at the bar of tests/test_remix_gpu.py."""
    from xumx_slicq_amd.separator import remix_gains
    sep = _sep("A", model)
    x = _input("A", 1, 2).cuda()
    G = remix_gains({"vocals": 0})
    got = sep.remix(x, {"vocals": 0})
    want = torch.einsum("rt,tbcn->rbcn", G.double(), sep(x).cpu().double())
    assert got.shape == want.shape == (1, 2, 2, x.shape[-1])
    d = got.cpu().double() - want
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    assert rms < RMS_TOL and mx < MAX_TOL, (model, rms, mx)


def test_no_iteration_is_the_mix_phase_model_and_two_iterations_agree_in_both_forms():
    """``niter = 0`` on the offline Wiener model is the offline mix-phase model bit for bit; ``niter = 2`` looped and
    window-resident are two summation orders of one filter, each held to float64 at fp32 rounding elsewhere
    (tests/test_wiener_iters_gpu.py): here 1e-5 of the stems' RMS, the bound that module holds its looped form to."""
    sep, mix = _sep("A", "offline_wiener"), _sep("A", "offline_phasemix")
    x = _input("A", 1, 2).cuda()
    try:
        sep.niter = 0
        assert torch.equal(sep(x), mix(x))
        sep.niter = 2
        out = {}
        for method in ("looped", "resident"):
            sep.xumx_model.niter_method = method
            out[method] = sep(x).cpu()
        e_rms, _ = ref64.rel_err(out["looped"], out["resident"].double())
        sep.niter = 1
        sep.xumx_model.niter_method = "auto"
        assert float(e_rms) < 1e-5 and not torch.equal(out["looped"], sep(x).cpu()), float(e_rms)
    finally:
        sep.niter = 1
        sep.xumx_model.niter_method = "auto"


@pytest.mark.parametrize("softmask,residual", [(1, 0), (0, 1), (1, 1)])
def test_softmask_and_residual_are_at_fp32_rounding_of_float64(softmask, residual):
    """Unmix.forward with the option set, one iteration, every block of A at S = 5, B = 2 with item 1 forty times louder, against
    the float64 closed form of tests/test_wiener_options_cpu.py (the generator of tests/golden/wiener_options.npz)."""
    sep = _sep("A", "offline_wiener")
    x = _input("A", 1, 2)
    x[1] *= 40.0
    X = sep.nsgt(x.cuda())
    kw = dict(softmask=bool(softmask), residual=bool(residual))
    try:
        sep.softmask, sep.residual = bool(softmask), bool(residual)
        Y, masks = sep.xumx_model(X, return_masks=True)
    finally:
        sep.softmask = sep.residual = False
    g, c = [], []
    for b in range(len(X)):
        Xb, mb = X[b].cpu(), masks[b].cpu()
        ref = wiener_options(Xb, mb.double() * ref64.abs_of_real_complex(Xb), 1, **kw)
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        c.append(ref64.rel_err(wiener_options(Xb, Ymag, 1, dtype=torch.complex64, **kw), wiener_options(Xb, Ymag, 1, **kw)))
        assert Y[b].shape[0] == 4 + residual
        g.append(ref64.rel_err(Y[b], ref))
    bad, _ = _judge("wiener_options", f"A S=5 B=2 softmask={softmask} residual={residual} niter=1", _pair(g), _pair(c), _labels("A", 5), full_table=True)
    assert not bad, "\n".join(bad)


# ---- 6. what stays refused ---------------------------------------------------------------------------------------------------------------
def test_stream_trainer_and_demix_into_refuse_before_any_launch():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.training import Trainer
    sep = _sep("A", "realtime")
    n = lengths(pkg_plan("A"))[0]
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        with pytest.raises(_lib.XsqError, match="long_bands"):
            sep.stream()
        with pytest.raises(_lib.XsqError, match="long_bands"):
            Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), precision="fp32")
        with pytest.raises(_lib.XsqError, match="long_bands"):
            sep.demix_into(audio(n, 2)[None].cuda(), torch.empty(4, 1, 2, n, device="cuda"), torch.zeros(4, 1, 2, dtype=torch.int64, device="cuda"))
        assert not _lib.profile_read(), _lib.profile_read()
    finally:
        _lib.profile_enable(False)
