"""More than one Wiener-EM iteration (``niter``) on the GPU: the looped and the window-resident form of every block against the
float64 k-iteration helper (tests/test_wiener_iters_cpu.py: one scaling, k applications of ``omodel._em_one_iteration`` in
complex128), window geometry, the separator end to end, the graph path, determinism, and that ``niter`` <= 1 runs what it ran.

The parity tests follow the rule of tests/test_ref64_gpu.py (``oracle.parity.Tables``):  e_gpu <= M * E  with E the LARGEST error
of the fp32 CPU helper (the same loop in complex64) over the blocks of the case, both by ``ref64.rel_err``; M is one power of two
per (stage, method), the smallest that is at least twice the worst e_gpu / E measured on MI355X, never above 16.  The measured
tables are in profiles/wiener_iters_parity.json, the worst ratio behind every M in DESIGN.md section 4.8.
"""
import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import ref64
from oracle.parity import M_CAP, Tables
from test_wiener_iters_cpu import wiener_iters
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
RMS_TOL, MAX_TOL = 1e-4, 1e-3

# (stage, method) -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/wiener_iters_parity.json)
M = {
    "wiener_iters/masked": 2,      # 0.80  (Unmix.forward = masked resident, n = 150,000, niter = 2, block 1)
    "wiener_iters/looped": 4,      # 1.08  (n = 9031, niter = 2, block 69, whole row in one window)
    "wiener_iters/resident": 4,    # 1.24  (n = 9031, niter = 2, block 69, win_len = 97)
    "stems_iters": 2,              # 0.93  (n = 100,000, niter = 2, stem 3)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("wiener_iters_parity", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


@pytest.fixture(scope="module")
def sep():
    from xumx_slicq_amd.separator import seeded_separator
    s = seeded_separator(realtime=False)
    yield s
    s.drop_graphs()


@pytest.fixture(autouse=True)
def _restore(sep):
    yield
    sep.niter, sep.chunk_size, sep.max_item_slices = 1, 2621440, 0
    sep.xumx_model.niter_method = "auto"
    sep.__dict__.pop("native", None)


@pytest.fixture(scope="module")
def em_inputs(sep):
    """n = 150,000, B = 2, batch row 1 forty times louder (S = 18): the mix coefficients and the sigmoid masks of every block."""
    n = 150000
    x = synth_audio(n, seed=20260101 + n, nb_samples=2)
    x[1] *= 40.0
    X = sep.nsgt(x.cuda())
    _, masks = sep.xumx_model(X, return_masks=True)
    assert X[0].shape[3] == 18
    return X, masks


def _pair(v):
    return tuple(np.array([float(e[i]) for e in v]) for i in (0, 1))


# ---- 1. every block at fp32 rounding ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter,blocks", [(2, tuple(range(70))), (5, (0, 1, 2, 4, 33, 69))])
def test_iterations_of_every_block_are_at_fp32_rounding_of_float64(sep, oracle_plan, em_inputs, niter, blocks):
    """Real block shapes at S = 18: blocks with T >= 280 have a full 5000-frame window and a tail of 40 to 256 frames, the window
    maximum is shared over the batch.  (a) the masked form the separator runs (Unmix.forward, auto = resident), (b) / (c) the
    module-level ``blockwise_wiener`` on the same initial magnitudes with method = "looped" / "resident"."""
    from xumx_slicq_amd.phase import blockwise_wiener
    X, masks = em_inputs
    assert any(18 * T > 5000 and (18 * T) % 5000 for (_, F, T) in oracle_plan.blocks)
    sep.xumx_model.niter = niter
    Y = sep.xumx_model(X)
    sep.xumx_model.niter = 1
    labels = [f"block {b} F {oracle_plan.blocks[b][1]} T {oracle_plan.blocks[b][2]} windows {-(-(18 * oracle_plan.blocks[b][2]) // 5000)}"
              for b in blocks]
    g = {"masked": [], "looped": [], "resident": []}
    c = []
    for b in blocks:
        Xb, mb = X[b].cpu(), masks[b].cpu()
        ref = wiener_iters(Xb, mb.double() * ref64.abs_of_real_complex(Xb), niter)
        Ymag = mb * omodel.abs_of_real_complex(Xb)                      # fp32: what the CPU helper and the module call start from
        ref_m = wiener_iters(Xb, Ymag, niter)
        c.append(ref64.rel_err(wiener_iters(Xb, Ymag, niter, dtype=torch.complex64), ref_m))
        g["masked"].append(ref64.rel_err(Y[b], ref))
        for method in ("looped", "resident"):
            g[method].append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), niter=niter, method=method), ref_m))
    bad = []
    for method, e in g.items():
        b_, _ = _T.judge("wiener_iters", f"n=150000 B=2 niter={niter} {method}", _pair(e), _pair(c), labels, full_table=True, arm=method)
        bad += [f"{method} {m}" for m in b_]
    assert not bad, "\n".join(bad)


# ---- 2. nothing moved -----------------------------------------------------------------------------------------------------------
def test_one_iteration_and_none_are_what_they_were(sep):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.phase import blockwise_phasemix_sep, blockwise_wiener
    from xumx_slicq_amd.separator import seeded_separator
    x = synth_audio(60000 * 2 + 30000, seed=93).cuda()
    sep.chunk_size = 60000
    default = sep(x).clone()
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        sep.niter = 1
        one = sep(x).clone()
        torch.cuda.synchronize()
        names1 = set(_lib.profile_read())
        _lib.profile_reset()
        sep.niter = 2
        two = sep(x).clone()
        torch.cuda.synchronize()
        names2 = set(_lib.profile_read())
    finally:
        _lib.profile_enable(False)
    assert torch.equal(default, one)
    new = {"wiener_resident", "wiener_stats_iter"}
    assert not (names1 & new) and "wiener_stats" in names1, names1            # niter = 1 runs the three launches it ran
    assert "wiener_resident" in names2 and "wiener_stats" not in names2, names2
    sep.niter = 0
    zero = sep(x).clone()
    pm = seeded_separator(realtime=False, wiener=False)
    pm.chunk_size = 60000
    assert torch.equal(zero, pm(x))
    d = float((two.double() - one.double()).pow(2).mean().sqrt() / one.double().pow(2).mean().sqrt())
    assert d > 1e-2, d
    # module level: niter = 1 is the call without it, whatever the method
    Xc = sep.nsgt(x[..., :60000])
    Xb = Xc[40]
    Ymag = torch.rand(4, *Xb.shape[:-1], device="cuda") * torch.sqrt(Xb[..., 0] ** 2 + Xb[..., 1] ** 2)
    base = blockwise_wiener(Xb, Ymag)
    for method in ("auto", "looped", "resident"):
        assert torch.equal(blockwise_wiener(Xb, Ymag, niter=1, method=method), base)
    assert torch.equal(blockwise_wiener(Xb, Ymag, niter=0), blockwise_phasemix_sep(Xb, Ymag))


# ---- 3. window geometry ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_inputs(sep):
    """n = 9031 (S = 3), B = 2, row 1 forty times louder."""
    x = synth_audio(9031, seed=20260101 + 9031, nb_samples=2)
    x[1] *= 40.0
    X = sep.nsgt(x.cuda())
    _, masks = sep.xumx_model(X, return_masks=True)
    assert X[0].shape[3] == 3
    return X, masks


@pytest.mark.parametrize("method", ["looped", "resident"])
def test_window_geometry(sep, oracle_plan, small_inputs, method):
    """S = 3, niter = 2: win_len = 100 (several windows and a tail per row; rows shorter than one window), win_len = 97 on the
    unmasked entry point (an odd window and an odd tail), win_len = 0 (the whole row), and the masked entry point at win_len = 100
    on the blocks whose rows have an even frame count."""
    from xumx_slicq_amd.arena import BlockTable
    from xumx_slicq_amd.phase import blockwise_wiener, wiener_em_masked_arena
    X, masks = small_inputs
    blocks = [0, 20, 33, 50, 68, 69]
    g, c, labels = [], [], []
    for b in blocks:
        _, F, T = oracle_plan.blocks[b]
        Xb, mb = X[b].cpu(), masks[b].cpu()
        Ymag = mb * omodel.abs_of_real_complex(Xb)
        for wl in (100, 97, 0):
            ref = wiener_iters(Xb, Ymag, 2, win_len=wl)
            c.append(ref64.rel_err(wiener_iters(Xb, Ymag, 2, win_len=wl, dtype=torch.complex64), ref))
            g.append(ref64.rel_err(blockwise_wiener(X[b], Ymag.cuda(), wl, niter=2, method=method), ref))
            labels.append(f"block {b} N {3 * T} win {wl}")
        if (3 * T) % 2 == 0:
            ref = wiener_iters(Xb, mb.double() * ref64.abs_of_real_complex(Xb), 2, win_len=100)
            Y = torch.empty(4, *Xb.shape, device="cuda")
            wiener_em_masked_arena(BlockTable([(F, T)]), X[b].contiguous().view(-1), masks[b].contiguous().view(-1), Y.view(-1), 2, 3,
                                   win_len=100, niter=2, method=method)
            c.append(ref64.rel_err(wiener_iters(Xb, Ymag, 2, win_len=100, dtype=torch.complex64), wiener_iters(Xb, Ymag, 2, win_len=100)))
            g.append(ref64.rel_err(Y, ref))
            labels.append(f"block {b} N {3 * T} win 100 masked")
    assert any("masked" in l for l in labels) and any(3 * oracle_plan.blocks[b][2] < 97 for b in blocks)
    bad, _ = _T.judge("wiener_iters", f"n=9031 B=2 niter=2 geometry {method}", _pair(g), _pair(c), labels, full_table=True, arm=method)
    assert not bad, "\n".join(bad)


# ---- 4. a window above the resident bound -------------------------------------------------------------------------------------
def test_window_above_the_resident_bound(sep, oracle_plan, em_inputs):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.phase import blockwise_wiener, resident_max_window
    X, masks = em_inputs
    T = oracle_plan.blocks[69][2]
    assert 18 * T == 5256 > resident_max_window() >= 5000
    Ymag = masks[69] * torch.sqrt(X[69][..., 0] ** 2 + X[69][..., 1] ** 2)
    auto = blockwise_wiener(X[69], Ymag, 0, niter=2, method="auto")
    looped = blockwise_wiener(X[69], Ymag, 0, niter=2, method="looped")
    assert torch.equal(auto, looped)
    ref = wiener_iters(X[69].cpu(), Ymag.cpu(), 2, win_len=0)
    assert float(ref64.rel_err(looped, ref)[0]) < 1e-5
    with pytest.raises(_lib.XsqError, match="resident"):
        blockwise_wiener(X[69], Ymag, 0, niter=2, method="resident")


# ---- 5. the separator end to end ------------------------------------------------------------------------------------------------
def test_split_batch_and_module_schedule_are_bitwise_the_native_call(sep):
    """The shape of test_batch_larger_than_one_pass_is_split_over_the_samples at niter = 2: nb = 5, chunks of 60,000, sample 3
    forty times louder, 20 item-slices per pass -- the passes of a set share the window maxima (ext_max of the resident kernel)."""
    x = synth_audio(60000 * 2 + 30000, seed=93, nb_samples=5).cuda()
    x[3] *= 40.0
    sep.niter = 2
    sep.chunk_size = 60000
    a = sep(x)
    sep.max_item_slices = 20
    b = sep(x)
    sep.native = False
    c = sep(x)
    assert torch.equal(a, b) and torch.equal(a, c)
    sep.niter = 1
    assert not torch.equal(a, sep(x))


def _separate_k(plan, sd, audio, k, f64):
    """One chunk, offline model, k EM iterations: float64 (ref64) or the fp32 CPU oracle with the fp32 helper."""
    from oracle import slicqt as oslicqt
    with torch.no_grad():
        if f64:
            Xl = ref64.forward(plan, audio.to(torch.float64))
        else:
            Xl = oslicqt.forward(plan, audio)
        Ys = []
        for b, Xb in enumerate(Xl):
            if f64:
                mag = ref64.abs_of_real_complex(Xb)
                m = ref64.cdae_masks(sd, b, mag, False)
                Ys.append(wiener_iters(Xb, m * mag, k))
            else:
                mag = omodel.abs_of_real_complex(Xb)
                m = omodel.cdae_masks(sd, b, mag, False)
                Ys.append(wiener_iters(Xb, m * mag, k, dtype=torch.complex64))
        return (ref64.inverse if f64 else oslicqt.inverse)(plan, Ys, audio.shape[-1])


def test_stems_of_two_iterations_are_at_fp32_rounding_of_float64(sep, oracle_plan, seeded_sd):
    n = 100000
    x = synth_audio(n, seed=20260101 + n)
    sep.niter = 2
    est = sep(x.cuda()).cpu()
    ref = _separate_k(oracle_plan, seeded_sd, x, 2, True)
    orc = _separate_k(oracle_plan, seeded_sd, x, 2, False)
    assert est.shape == ref.shape == (4, 1, 2, n)
    d = est.double() - ref
    rms, mx = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    print(f"stems niter=2 n={n}: rms {rms:.3e} max {mx:.3e}")
    assert rms < RMS_TOL and mx < MAX_TOL, (rms, mx)
    bad, _ = _T.judge("stems_iters", f"offline niter=2 n={n}", ref64.rel_err(est, ref, keep=(0,)), ref64.rel_err(orc, ref, keep=(0,)),
                      [f"stem {t}" for t in range(4)], full_table=True)
    assert not bad, "\n".join(bad)


def test_remix_follows_the_iteration_count(sep):
    """Karaoke through ``remix`` against the gain-weighted sum of ``forward``'s stems (the comparison of tests/test_remix_gpu.py)."""
    x = synth_audio(60000 * 2 + 777, seed=92, nb_samples=2).cuda()
    sep.niter = 2
    sep.chunk_size = 60000
    stems = sep(x)
    got = sep.remix(x, {"vocals": 0})
    G = [[1.0, 0.0, 1.0, 1.0]]
    ref = torch.einsum("rt,tbcn->rbcn", torch.tensor(G, dtype=torch.float64), stems.double().cpu())
    d = got.double().cpu() - ref
    rms = float(d.pow(2).mean().sqrt()) / float(ref.pow(2).mean().sqrt())
    mx = float(d.abs().max()) / float(ref.abs().max())
    assert got.shape == (1, 2, 2, x.shape[-1]) and rms < 2e-6 and mx < 2e-5, (rms, mx)
    sep.niter = 1
    assert not torch.equal(got, sep.remix(x, {"vocals": 0}))


# ---- 6. the graph path ------------------------------------------------------------------------------------------------------------
def test_graph_replay_follows_the_iteration_count(sep):
    sep.chunk_size = 60000
    a = synth_audio(150000, seed=41).cuda()
    try:
        sep.niter = 2
        e2 = sep(a).clone()
        g2 = sep.forward_graphed(a).clone()
        g2b = sep.forward_graphed(a).clone()             # a replay
        sep.niter = 1
        e1 = sep(a).clone()
        g1 = sep.forward_graphed(a).clone()              # same shape, another count: not the old graph
        sep.niter = 2
        g2c = sep.forward_graphed(a).clone()
    finally:
        sep.drop_graphs()
    assert torch.equal(e2, g2) and torch.equal(e2, g2b) and torch.equal(e1, g1) and torch.equal(e2, g2c)
    assert not torch.equal(e1, e2)


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------
def test_three_iterations_twice_are_bitwise_equal(sep, em_inputs):
    from xumx_slicq_amd.phase import blockwise_wiener
    x = synth_audio(60000 * 2 + 30000, seed=7, nb_samples=2).cuda()
    sep.niter = 3
    sep.chunk_size = 60000
    a = sep(x).clone()
    b = sep(x).clone()
    assert torch.equal(a, b)
    X, masks = em_inputs
    Ymag = masks[69] * torch.sqrt(X[69][..., 0] ** 2 + X[69][..., 1] ** 2)
    for method in ("looped", "resident"):
        assert torch.equal(blockwise_wiener(X[69], Ymag, niter=3, method=method), blockwise_wiener(X[69], Ymag, niter=3, method=method))


# ---- 8. training differentiates one iteration -------------------------------------------------------------------------------------
def test_trainer_refuses_more_than_one_iteration(sep):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.training import Trainer
    sep.niter = 2
    with pytest.raises(_lib.XsqError, match="ONE Wiener-EM iteration"):
        Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm))
