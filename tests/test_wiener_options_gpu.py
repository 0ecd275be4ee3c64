"""The Wiener filter's option sets (``softmask``, ``residual``) on the GPU: every form against the float64 helper of
tests/test_wiener_options_cpu.py (the reference's norbert semantics with float32 epsilons), window geometry, ``niter`` = 0, the
separator end to end, that the paths agree bit for bit, that nothing moves with both flags off, and the refusals.

The parity tests follow the rule of tests/test_wiener_iters_gpu.py (``oracle.parity.Tables``):  e_gpu <= M * E  with E the LARGEST
error of the complex64 CPU helper over the case, both by ``ref64.rel_err``; M is one power of two per (stage, method), the smallest
that is at least twice the worst e_gpu / E measured on MI355X, never above 16.  The measured tables are in
profiles/wiener_options_parity.json, the worst ratio behind every M in DESIGN.md section 4.10.

The sigmoid masks of the seeded model sum above 1 at more than nine points in ten, where the residual is zero.  The parity tests
therefore run on a model whose last-layer biases are lowered by ``MASK_LOGIT_SHIFT`` -- on both sides: the CPU references take the
masks, or the parameters, of that same model -- and assert the share of points with a positive residual.
"""
import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import ref64
from oracle.parity import M_CAP, Tables
from test_wiener_options_cpu import EPS, wiener_options
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3
MASK_LOGIT_SHIFT = 1.5          # share of points with sum_j m_j < 1 on the CPU oracle: 0.07 - 0.09 without, 0.30 - 0.36 with it
OPTION_SETS = ((0, 1, 1), (1, 0, 1), (1, 1, 2), (0, 1, 3))                     # (softmask, residual, niter)
FLAG_PAIRS = ((1, 0), (0, 1), (1, 1))

# (stage, method) -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/wiener_options_parity.json)
M = {
    "wiener_options/masked": 2,      # 0.79  (Unmix.forward, n = 150,000, softmask + residual, niter = 2, block 1)
    "wiener_options/looped": 2,      # 0.93  (n = 150,000, softmask + residual, niter = 2, block 1)
    "wiener_options/resident": 2,    # 0.91  (n = 9031, softmask + residual, niter = 2, block 20, win_len = 100, from masks)
    "wiener_options/start": 4,       # 1.04  (n = 9031, softmask + residual, niter = 0, block 69, from masks)
    "stems_options": 4,              # 1.30  (n = 100,000, softmask + residual, niter = 1, stem 1)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("wiener_options_parity", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


@pytest.fixture(scope="module")
def sep():
    """The seeded offline separator with every last-layer bias lowered by MASK_LOGIT_SHIFT."""
    from xumx_slicq_amd.separator import seeded_separator
    s = seeded_separator(realtime=False)
    with torch.no_grad():
        for blk in s.xumx_model.sliced_umx:
            for cdae in blk.cdaes:
                cdae[9].bias -= MASK_LOGIT_SHIFT
    s.xumx_model.refresh()
    yield s
    s.drop_graphs()


@pytest.fixture(autouse=True)
def _restore(sep):
    yield
    sep.niter, sep.softmask, sep.residual, sep.chunk_size, sep.max_item_slices = 1, False, False, 2621440, 0
    sep.xumx_model.niter_method = "auto"
    sep.__dict__.pop("native", None)


def _inputs(sep, n):
    x = synth_audio(n, seed=20260101 + n, nb_samples=2)
    x[1] *= 40.0
    X = sep.nsgt(x.cuda())
    _, masks = sep.xumx_model(X, return_masks=True)
    return X, masks


@pytest.fixture(scope="module")
def em_inputs(sep):
    """n = 150,000, B = 2, batch row 1 forty times louder (S = 18): the mix coefficients and the sigmoid masks of every block."""
    X, masks = _inputs(sep, 150000)
    assert X[0].shape[3] == 18
    return X, masks


@pytest.fixture(scope="module")
def small_inputs(sep):
    """n = 9031 (S = 3), B = 2, row 1 forty times louder."""
    X, masks = _inputs(sep, 9031)
    assert X[0].shape[3] == 3
    return X, masks


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


def _residual_share(pairs):
    """Share of the points (block, item, channel, bin, frame) of [(X block, masks block)] whose residual magnitude is positive."""
    pos = tot = 0
    for Xb, mb in pairs:
        ax = omodel.abs_of_real_complex(Xb)
        v = mb * ax
        vr = torch.where(ax > EPS, ax, torch.full_like(ax, EPS)) - (((v[0] + v[1]) + v[2]) + v[3])
        pos, tot = pos + int((vr > 0).sum()), tot + vr.numel()
    return pos / tot


def _set(sep, softmask, residual, niter):
    sep.softmask, sep.residual, sep.niter = bool(softmask), bool(residual), niter


# ---- 1. full windows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("softmask,residual,niter", OPTION_SETS)
def test_option_sets_are_at_fp32_rounding_of_float64(sep, oracle_plan, em_inputs, softmask, residual, niter):
    """Real block shapes at S = 18 (full 5000-frame windows and tails; the window maximum shared over the batch).  (a) the masked
    form the separator runs (Unmix.forward), (b) / (c) the module-level ``blockwise_wiener`` on the same fp32 magnitudes with
    method = "looped" / "resident".  At five sources the resident kernel holds shorter windows: where the default window does not
    fit, that arm runs -- on both sides -- with windows of ``resident_max_window(5)`` frames."""
    from xumx_slicq_amd.phase import blockwise_wiener, resident_max_window
    X, masks = em_inputs
    blocks = (0, 1, 2, 4, 33, 69)
    assert any(18 * oracle_plan.blocks[b][2] > 5000 and (18 * oracle_plan.blocks[b][2]) % 5000 for b in blocks)
    share = _residual_share([(X[b].cpu(), masks[b].cpu()) for b in blocks])
    print(f"share of points with a positive residual: {share:.3f} (mask logit shift {MASK_LOGIT_SHIFT})")
    assert 0.1 <= share <= 0.9, share
    _set(sep, softmask, residual, niter)
    Y = sep.xumx_model(X)
    _set(sep, 0, 0, 1)
    kw = dict(softmask=bool(softmask), residual=bool(residual))
    J = 4 + residual
    wres = resident_max_window(J)
    g = {"masked": [], "looped": [], "resident": []}
    c, labels = [], []
    for b in blocks:
        _, F, T = oracle_plan.blocks[b]
        Xb, mb = X[b].cpu(), masks[b].cpu()
        assert Y[b].shape == (J, *Xb.shape)
        ref = wiener_options(Xb, mb.double() * ref64.abs_of_real_complex(Xb), niter, **kw)
        Ymag = mb * omodel.abs_of_real_complex(Xb)                      # fp32: what the CPU helper and the module call start from
        ref_m = wiener_options(Xb, Ymag, niter, **kw)
        c.append(ref64.rel_err(wiener_options(Xb, Ymag, niter, dtype=torch.complex64, **kw), ref_m))
        g["masked"].append(ref64.rel_err(Y[b], ref))
        g["looped"].append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), niter=niter, method="looped", **kw), ref_m))
        wl = 5000 if min(5000, 18 * T) <= wres else wres
        ref_r = ref_m if wl == 5000 else wiener_options(Xb, Ymag, niter, win_len=wl, **kw)
        g["resident"].append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), wl, niter=niter, method="resident", **kw), ref_r))
        labels.append(f"block {b} F {F} T {T} windows {-(-(18 * T) // 5000)}" + ("" if wl == 5000 else f" (resident: {wl})"))
    bad = []
    for method, e in g.items():
        b_, _ = _T.judge("wiener_options", f"n=150000 B=2 softmask={softmask} residual={residual} niter={niter} {method}", _pair(e), _pair(c),
                         labels, full_table=True, arm=method)
        bad += [f"{method} {m}" for m in b_]
    assert not bad, "\n".join(bad)


# ---- 2. window geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["looped", "resident"])
def test_window_geometry(sep, oracle_plan, small_inputs, method):
    """S = 3, softmask + residual, niter = 2: win_len = 100 (several windows and a tail per row; rows shorter than one window),
    win_len = 97 on the unmasked entry point (an odd window and an odd tail), win_len = 0 (the whole row), and the masked entry point
    at win_len = 100 on the blocks whose rows have an even frame count."""
    from xumx_slicq_amd.arena import BlockTable
    from xumx_slicq_amd.phase import blockwise_wiener, wiener_em_masked_arena
    X, masks = small_inputs
    blocks = [0, 20, 33, 50, 68, 69]
    kw = dict(softmask=True, residual=True)
    g, c, labels = [], [], []
    for b in blocks:
        _, F, T = oracle_plan.blocks[b]
        Xb, mb = X[b].cpu(), masks[b].cpu()
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        for wl in (100, 97, 0):
            ref = wiener_options(Xb, Ymag, 2, win_len=wl, **kw)
            c.append(ref64.rel_err(wiener_options(Xb, Ymag, 2, win_len=wl, dtype=torch.complex64, **kw), ref))
            g.append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), wl, niter=2, method=method, **kw), ref))
            labels.append(f"block {b} N {3 * T} win {wl}")
        if (3 * T) % 2 == 0:
            ref = wiener_options(Xb, mb.double() * ref64.abs_of_real_complex(Xb), 2, win_len=100, **kw)
            Y = torch.empty(5, *Xb.shape, device="cuda")
            wiener_em_masked_arena(BlockTable([(F, T)]), X[b].contiguous().view(-1), masks[b].contiguous().view(-1), Y.view(-1), 2, 3,
                                   win_len=100, niter=2, method=method, **kw)
            c.append(ref64.rel_err(wiener_options(Xb, Ymag, 2, win_len=100, dtype=torch.complex64, **kw), wiener_options(Xb, Ymag, 2, win_len=100, **kw)))
            g.append(ref64.rel_err(Y, ref))
            labels.append(f"block {b} N {3 * T} win 100 masked")
    assert any("masked" in l for l in labels) and any(3 * oracle_plan.blocks[b][2] < 97 for b in blocks)
    bad, _ = _T.judge("wiener_options", f"n=9031 B=2 softmask=1 residual=1 niter=2 geometry {method}", _pair(g), _pair(c), labels,
                      full_table=True, arm=method)
    assert not bad, "\n".join(bad)


# ---- 3. niter = 0: the starts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("softmask,residual", FLAG_PAIRS)
def test_no_iteration_returns_the_start(sep, oracle_plan, small_inputs, softmask, residual):
    """The J initial estimates, unscaled, from magnitudes (``blockwise_wiener``) and from the masks (``wiener_em_masked_arena``), with
    a few coefficients of the mix set to zero first: a silent point's targets are 0 and its
    residual is eps, real (angle(0) = 0), from the mixture phase and 0 from the ratio mask."""
    from xumx_slicq_amd.arena import BlockTable
    from xumx_slicq_amd.phase import blockwise_wiener, wiener_em_masked_arena
    X, masks = small_inputs
    kw = dict(softmask=bool(softmask), residual=bool(residual))
    J = 4 + residual
    g, c, labels = [], [], []
    for b in (0, 20, 33, 50, 68, 69):
        _, F, T = oracle_plan.blocks[b]
        Xg = X[b].clone()
        Xg[:, :, :, 1, 3:6] = 0.0                        # three frames silent in both channels
        Xg[:, 1, :, 2, 7] = 0.0                          # one frame silent in channel 1
        Xb, mb = Xg.cpu(), masks[b].cpu()
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        ref_m = wiener_options(Xb, Ymag, 0, **kw)
        e_cpu = ref64.rel_err(wiener_options(Xb, Ymag, 0, dtype=torch.complex64, **kw), ref_m)
        got = blockwise_wiener(Xg, Ymag.cuda(), niter=0, **kw)
        assert got.shape == (J, *Xb.shape) and bool(torch.isfinite(got).all())
        if residual:                                     # (the ratio mask multiplies x = 0; the mixture phase of 0 is 1)
            assert torch.equal(got[4, :, :, :, 1, 3:6].cpu(), torch.tensor([0.0 if softmask else EPS, 0.0]).expand(2, 2, F, 3, 2))
        assert not bool(got[:4, :, :, :, 1, 3:6].any())
        g.append(ref64.rel_err(got, ref_m)); c.append(e_cpu); labels.append(f"block {b} N {3 * T} magnitudes")
        if (3 * T) % 2 == 0:
            Y = torch.empty(J, *Xb.shape, device="cuda")
            wiener_em_masked_arena(BlockTable([(F, T)]), Xg.contiguous().view(-1), masks[b].contiguous().view(-1), Y.view(-1), 2, 3,
                                   niter=0, **kw)
            g.append(ref64.rel_err(Y, wiener_options(Xb, mb.double() * ref64.abs_of_real_complex(Xb), 0, **kw)))
            c.append(e_cpu); labels.append(f"block {b} N {3 * T} masks")
    bad, _ = _T.judge("wiener_options", f"n=9031 B=2 softmask={softmask} residual={residual} niter=0", _pair(g), _pair(c), labels,
                      full_table=True, arm="start")
    assert not bad, "\n".join(bad)


# ---- 4. nothing moved -----------------------------------------------------------------------------------------------------------
# the profile names of a default forward (offline model, one iteration, three chunks): the launches of the commit before the options
DEFAULT_FORWARD_PROFILE = {"band_analysis_dft4", "band_analysis_gemm", "band_synthesis_dft4", "band_synthesis_gemm", "cdae_l1_gemm",
                           "cdae_l2_gemm", "cdae_l3_gemm", "cdae_l4_gemm", "slice_irfft_ola", "slice_rfft", "wiener_apply", "wiener_finalize",
                           "wiener_stats"}


def test_flags_off_is_what_it_was():
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import seeded_separator
    x = synth_audio(150000, seed=93, nb_samples=2).cuda()
    plain = seeded_separator(realtime=False)
    for name in ("softmask", "residual"):
        del plain.xumx_model.__dict__[name]                              # a model that never had the attributes
    off = seeded_separator(realtime=False, softmask=False, residual=False)
    for s in (plain, off):
        s.chunk_size = 60000
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        a = off(x)
        torch.cuda.synchronize()
        names = set(_lib.profile_read())
    finally:
        _lib.profile_enable(False)
    print("profile names of a default forward:", sorted(names))
    assert names == DEFAULT_FORWARD_PROFILE, names ^ DEFAULT_FORWARD_PROFILE
    assert a.shape == (4, 2, 2, 150000) and torch.equal(a, plain(x))
    assert torch.equal(off.remix(x, {"vocals": 0}), plain.remix(x, {"vocals": 0}))
    assert torch.equal(off.forward_overlapped(x, 0.25, 0.05), plain.forward_overlapped(x, 0.25, 0.05))
    for opt in ("softmask", "residual"):
        setattr(off, opt, True)
        b = off(x)
        setattr(off, opt, False)
        d = float((b[:4].double() - a.double()).pow(2).mean().sqrt() / a.double().pow(2).mean().sqrt())
        print(f"{opt}: relative rms distance of the four targets from the default {d:.3e}")
        assert b.shape[0] == (5 if opt == "residual" else 4) and d > 1e-3, (opt, d)
    assert torch.equal(off(x), a)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def _separate(plan, sd, audio, f64):
    """One chunk, offline model, softmask + residual, one iteration: float64 (ref64) or the fp32 CPU oracle with the complex64 helper."""
    from oracle import slicqt as oslicqt
    with torch.no_grad():
        Xl = ref64.forward(plan, audio.to(torch.float64)) if f64 else oslicqt.forward(plan, audio)
        Ys, pairs = [], []
        for b, Xb in enumerate(Xl):
            if f64:
                mag = ref64.abs_of_real_complex(Xb)
                m = ref64.cdae_masks(sd, b, mag, False)
                Ys.append(wiener_options(Xb, m * mag, 1, True, True))
            else:
                mag = omodel.abs_of_real_complex(Xb)
                m = omodel.cdae_masks(sd, b, mag, False)
                Ys.append(wiener_options(Xb, m * mag, 1, True, True, dtype=torch.complex64))
                pairs.append((Xb, m))
        return (ref64.inverse if f64 else oslicqt.inverse)(plan, Ys, audio.shape[-1]), pairs


def test_five_stems_are_at_fp32_rounding_of_float64(sep, oracle_plan):
    n = 100000
    x = synth_audio(n, seed=20260101 + n)
    sd = {k: v.detach().cpu() for k, v in sep.xumx_model.state_dict().items()}
    _set(sep, 1, 1, 1)
    est = sep(x.cuda()).cpu()
    ref, _ = _separate(oracle_plan, sd, x, True)
    orc, pairs = _separate(oracle_plan, sd, x, False)
    share = _residual_share(pairs)
    print(f"share of points with a positive residual: {share:.3f}")
    assert 0.1 <= share <= 0.9, share
    assert est.shape == ref.shape == (5, 1, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    print(f"stems softmask residual niter=1 n={n}: rms {rms:.3e} max {mx:.3e}")
    assert rms < RMS_TOL and mx < MAX_TOL, (rms, mx)
    bad, _ = _T.judge("stems_options", f"offline softmask=1 residual=1 niter=1 n={n}", ref64.rel_err(est, ref, keep=(0,)),
                      ref64.rel_err(orc, ref, keep=(0,)), [f"stem {t}" for t in range(5)], full_table=True)
    assert not bad, "\n".join(bad)


# ---- 6. the paths agree -----------------------------------------------------------------------------------------------------------
def test_split_batch_and_module_schedule_are_bitwise_the_native_call(sep):
    x = synth_audio(60000 * 2 + 30000, seed=93, nb_samples=5).cuda()
    x[3] *= 40.0
    _set(sep, 0, 1, 2)
    sep.chunk_size = 60000
    a = sep(x)
    b = sep(x)                                           # two runs
    sep.max_item_slices = 20
    c = sep(x)
    sep.native = False
    d = sep(x)
    assert a.shape == (5, 5, 2, x.shape[-1])
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_graph_replay_is_keyed_by_the_flags(sep):
    sep.chunk_size = 60000
    a = synth_audio(150000, seed=41).cuda()
    try:
        _set(sep, 1, 1, 1)
        e11 = sep(a).clone()
        g11 = sep.forward_graphed(a).clone()
        g11b = sep.forward_graphed(a).clone()            # a replay
        _set(sep, 1, 0, 1)
        e10 = sep(a).clone()
        g10 = sep.forward_graphed(a).clone()             # same shape, other flags: not the old graph
        _set(sep, 1, 1, 1)
        g11c = sep.forward_graphed(a).clone()
    finally:
        sep.drop_graphs()
    assert e11.shape[0] == 5 and e10.shape[0] == 4
    assert torch.equal(e11, g11) and torch.equal(e11, g11b) and torch.equal(e10, g10) and torch.equal(e11, g11c)


def test_overlapped_segments_carry_the_residual(sep):
    from xumx_slicq_amd.separator import segments
    x = synth_audio(40000, seed=17, nb_samples=2).cuda()
    _set(sep, 0, 1, 1)
    out = sep.forward_overlapped(x, 0.25, 0.05)
    assert out.shape == (5, 2, 2, 40000)
    chunk_len, ov = sep._segment_lengths(0.25, 0.05)
    segs = segments(40000, chunk_len, ov)
    assert len(segs) >= 3
    for start, n, fi, fo in segs:
        est = sep(x[..., start:start + n])
        assert torch.equal(out[..., start + fi:start + n - fo], est[..., fi:n - fo]), (start, n)


# ---- 7. refusals on the device --------------------------------------------------------------------------------------------------
def test_refusals(sep):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.training import Trainer
    x = synth_audio(30000, seed=5).cuda()
    sep.residual = True
    with pytest.raises(ValueError, match="residual"):
        sep.remix(x, {"vocals": 0})
    with pytest.raises(ValueError, match="residual"):
        sep.demix_into(x, torch.empty(4, 1, 2, 30000, device="cuda"), torch.zeros(4, 1, 2, dtype=torch.int64, device="cuda"))
    for opt in ("softmask", "residual"):
        _set(sep, opt == "softmask", opt == "residual", 1)
        with pytest.raises(_lib.XsqError, match=opt):
            Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm))
        rt = seeded_separator(realtime=True)
        setattr(rt, opt, True)
        with pytest.raises(_lib.XsqError, match=opt):
            rt(x)
    sep.residual, sep.softmask = False, True
    assert sep.remix(x, {"vocals": 0}).shape == (1, 1, 2, 30000)                 # remix does honour softmask
