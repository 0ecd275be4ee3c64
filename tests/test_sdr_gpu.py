"""The SDR loss term on the GPU at fp32 rounding of float64: the adjoint of the inverse sliCQT (xsq_slicqt_inverse_adjoint), the SD-SDR
criterion and its gradient (csrc/sdr.hip), the training step with the term (xsq_train_step_sdr through ``Trainer(sdr_mcoef=...)``), the
off switch and ``validation_step(sdr_mcoef=...)``.

Rule and metric are those of tests/test_ref64_gpu.py and tests/test_ref64_train_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err``, E the error
against float64 of the SAME closed forms evaluated in float32 / complex64 on the CPU on the same inputs (tests/test_sdr_cpu.py carries
them with a dtype), M a power of two <= M_CAP by the rule of DESIGN.md section 2 (smallest power of two >= twice the worst ratio measured
on MI355X).  The whole step is judged like tests/test_ref64_train_gpu.py judges it (same classes, ill-conditioned whitening rule and
near-kink rule: RISK, 15 % RMS for a loose tensor, at most 2 % loose per case); its float64 reference is one backward over all blocks
through masks -> post-filter -> inverse sliCQT -> SD-SDR formula, on the GPU's own coefficients of the batch.

The SD-SDR formula is the contract of DESIGN.md section 7 (auraloss is not installed anywhere this project runs)."""
import numpy as np
import pytest
import torch

from oracle import loss as oloss
from oracle import model as omodel
from oracle import ref64
from oracle.parity import M_CAP, Tables
from test_ref64_train_gpu import (BATCHES, CLASSES, GROUP, KINK_RTOL, LOOSE_SHARE, MODELS, RISK, _abs_err, _class, _coefficients, _sep,
                                  _trainer)
from test_sdr_cpu import (F32, F64, adjoint_closed_form, adjoint_window, autograd_adjoint, inverse_dtype, random_blocks, sdr_criterion)

pytestmark = pytest.mark.gpu

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_sdr_parity.json)
M = {
    "adjoint": 4,                  # 1.31  (Bark-262, BC 8, n = 9031: block 1, F 86, T 16; 1.15 accumulating onto a non-zero arena)
    "adjoint/rocfft": 4,           # 1.31  (Mel-32, BC 8, n = 32768: block 0, F 9, T 16)
    "sdr/loss": 1,                 # 0.003 (silent target: the moments are fp64 sums of exact products, the fp32 formula's are not)
    "sdr/gy": 2,                   # 0.85  (B 2, n = 9031, silent target: source 0, b 0, ch 1)
    "train/conv": 8,               # 2.46  (S3, causal + mix-phase: block 49 / target 0, 3.weight)
    "train/bn": 8,                 # 3.11  (same case: block 49 / target 0, 1.weight)
    "train/whiten": 16,            # 9.49  (same case: block 33, input_mean; twice that is past the cap, M is the cap.  1.77 and 1.00 in the other two cases.
                                   #        A one-bin block: the cancellation of DESIGN.md section 7, "The whitening class at 9.49", with the figures behind it)
    "train/loss": 2,               # 0.57  (same case; E is three scalars per case: 3.0e-7 .. 3.8e-7)
    "validation": 8,               # 2.15  (S3, offline + Wiener; E is three scalars: 3.3e-8)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("ref64_sdr_parity", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


def _bark_engine():
    return _sep(False).nsgt.nsgt.nsgt


_MEL = {}


def _mel():
    if not _MEL:
        from oracle import slicqt as O
        from xumx_slicq_amd.transforms import NSGTBase
        _MEL["plan"] = O.make_plan("mel", 32, 115.5)
        _MEL["eng"] = NSGTBase("mel", 32, 115.5, device="cuda").nsgt
    return _MEL["plan"], _MEL["eng"]


# ---- 1. the adjoint alone -----------------------------------------------------------------------------------------------
def _judge_adjoint(plan, eng, BC, n, stage, case, accumulate=False):
    gy, ref, S = autograd_adjoint(plan, BC, n, seed=BC * 1000 + n % 997)
    gy32 = gy.float()
    ref = [r for r in ref]
    cpu = adjoint_closed_form(plan, adjoint_window(plan), gy32, S, dtype=F32)
    base = None
    if accumulate:
        base = random_blocks(plan, BC, S, seed=99, dtype=F32)
        arena, _, _ = eng.table.as_arena([b.cuda() for b in base])
        arena = arena.clone()
        out = eng.backward_adjoint(gy32.cuda(), S, out=arena)
    else:
        out = eng.backward_adjoint(gy32.cuda(), S)
    got = [v.cpu() for v in eng.table.views(out, (BC,), S)]
    if accumulate:          # what was there plus the adjoint: judged on the sum's own scale, E with the same single fp32 addition
        ref = [r + b.double() for r, b in zip(ref, base)]
        cpu = [c + b for c, b in zip(cpu, base)]
    e_gpu = np.array([[float(v) for v in ref64.rel_err(g, r)] for g, r in zip(got, ref)]).T
    e_cpu = np.array([[float(v) for v in ref64.rel_err(c, r)] for c, r in zip(cpu, ref)]).T
    labels = [f"block {b} (F {F}, T {T})" for b, (_, F, T) in enumerate(plan.blocks)]
    bad, worst = _T.judge(stage, case, (e_gpu[0], e_gpu[1]), (e_cpu[0], e_cpu[1]), labels)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("BC,n,S", [(8, 9031, 3), (8, 44100, 6), (3, 70000, 9)])
def test_adjoint_of_every_block_is_at_fp32_rounding_of_float64_autograd(oracle_plan, BC, n, S):
    """Bark-262 (hand-written slice FFT, radix-4 and dense band kernels): the smallest and odd length (n % 4 == 3), both slice
    parities, and a row count that is no multiple of anything."""
    assert oracle_plan.nslices(n) == S
    _judge_adjoint(oracle_plan, _bark_engine(), BC, n, "adjoint", f"bark BC {BC} n {n}")


def test_adjoint_on_the_rocfft_path(oracle_plan):
    plan, eng = _mel()
    _judge_adjoint(plan, eng, 8, 32768, "adjoint/rocfft", "mel BC 8 n 32768")


def test_adjoint_accumulates_onto_a_nonzero_arena(oracle_plan):
    _judge_adjoint(oracle_plan, _bark_engine(), 8, 9031, "adjoint", "bark BC 8 n 9031 accumulate", accumulate=True)


# ---- 2. criterion and gy ------------------------------------------------------------------------------------------------
def _waveforms(B, n, seed, loud_row=False, silent=None):
    from xumx_slicq_amd.synth import synth_audio
    t = torch.stack([0.5 * synth_audio(n, seed=seed + j, nb_samples=B) for j in range(4)])
    p = 0.8 * t + 0.1 * torch.stack([synth_audio(n, seed=seed + 10 + j, nb_samples=B) for j in range(4)])
    if loud_row:
        t[:, 1] *= 40.0
        p[:, 1] *= 40.0
    if silent is not None:
        t[silent] = 0.0
    return p.contiguous(), t.contiguous()


def _sdr_reference(p, t, dtype):
    pp = p.to(dtype).clone().requires_grad_(True)
    loss, rows = sdr_criterion(pp, t, dtype)
    loss.backward()
    return float(loss.detach()), rows.detach(), pp.grad


def _judge_sdr(case, p, t):
    from xumx_slicq_amd.loss import SDRLossCriterion, sdr_loss_and_gradient
    l64, rows64, g64 = _sdr_reference(p, t, F64)
    l32, rows32, g32 = _sdr_reference(p, t, F32)
    out, gy = sdr_loss_and_gradient(p.cuda(), t.cuda())
    out, gy = out.cpu(), gy.cpu()
    B = p.shape[1]
    rows = out[1:1 + 28 * B].reshape(B, 2, 14).permute(2, 0, 1)
    assert torch.isfinite(out).all() and torch.isfinite(gy).all()
    fwd = float(SDRLossCriterion()(p.cuda(), t.cuda()))
    assert abs(fwd - float(out[0])) <= 1e-6 * abs(float(out[0]))                     # the forward-only entry point: the same passes
    # row losses: absolute error in dB relative to the RMS of the float64 row losses (rel_err), plus the criterion itself
    e_gpu = [np.array([a]) for a in ref64.rel_err(rows, rows64)]
    e_cpu = [np.array([a]) for a in ref64.rel_err(rows32, rows64)]
    bad, _ = _T.judge("sdr/loss", case, e_gpu, e_cpu, ["row losses"])
    print(f"  criterion {float(out[0]):.9f} (float64 {l64:.9f}, fp32 formula {l32:.9f})")
    if abs(float(out[0]) - l64) > M["sdr/loss"] * abs(l32 - l64):
        bad.append(f"criterion: {float(out[0]):.9e} vs {l64:.9e} (fp32 formula {l32:.9e})")
    eg, ec = ref64.rel_err(gy, g64, keep=(0, 1, 2)), ref64.rel_err(g32, g64, keep=(0, 1, 2))
    labels = [f"source {i} b {b} ch {c}" for i in range(4) for b in range(B) for c in range(2)]
    bad2, _ = _T.judge("sdr/gy", case, eg, ec, labels)
    assert not (bad + bad2), "\n".join((bad + bad2)[:20])
    return rows, gy, out[1 + 28 * B:].reshape(2, B, 2, 14)


def test_sdr_criterion_and_gradient_plain():
    _judge_sdr("B 1 n 9031", *_waveforms(1, 9031, 700))


def test_sdr_criterion_and_gradient_with_a_loud_row():
    """Row 1 forty times louder: a sum shared across rows would show."""
    _judge_sdr("B 2 n 44100 loud row", *_waveforms(2, 44100, 710, loud_row=True))


def test_sdr_criterion_and_gradient_with_a_silent_target():
    """Target 2 silent in row (b 1, ch 0): loss and gy finite and equal to float64; the silent single combination's row loss is
    -10 log10(eps) = 80 and the two scalars of its gradient  A t + B (p - t)  are exactly 0 (the other 13 combinations of the row
    have a gradient).  With all four targets of a row silent every combination of the row is: gy of that row is exactly 0."""
    p, t = _waveforms(2, 9031, 720, silent=(2, 1, 0))
    rows, _, AB = _judge_sdr("B 2 n 9031 silent target", p, t)
    assert abs(float(rows[2, 1, 0]) - 80.0) < 1e-9
    assert float(AB[0, 1, 0, 2]) == 0.0 and float(AB[1, 1, 0, 2]) == 0.0
    others = torch.ones(14, dtype=torch.bool)
    others[2] = False
    assert bool((AB[0, 1, 0, others] != 0).all()) and bool((AB[1, 1, 0, others] != 0).all()) and bool((AB[:, 0] != 0).all())
    from xumx_slicq_amd.loss import sdr_loss_and_gradient
    t[:, 0, 1] = 0.0
    out, gy = sdr_loss_and_gradient(p.cuda(), t.cuda())
    rows = out.cpu()[1:1 + 56].reshape(2, 2, 14)
    assert torch.isfinite(out).all() and torch.isfinite(gy).all()
    assert bool((rows[0, 1] - 80.0).abs().max() < 1e-9) and not bool(gy[:, 0, 1].any())


# ---- 3. the whole step --------------------------------------------------------------------------------------------------
_REF, _CASE = {}, {}


def step_reference(plan, sd, X, Yt, y_t, causal, wiener, mcoef, dtype):
    """One forward + ONE backward over all blocks of  mse + mask + mcoef * sdr  in ``dtype``: (mse, mask, sdr, grads, minima)."""
    nb, n = len(plan.blocks), y_t.shape[-1]
    p = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    p = {k: (v.clone().requires_grad_(True) if k.endswith(oloss.TRAINABLE_SUFFIXES) else v) for k, v in p.items()}
    minima, Ys = {}, []
    mse = msk = 0.0
    for b in range(nb):
        pre = f"sliced_umx.{b}."
        pb = {k: v for k, v in p.items() if k.startswith(pre)}
        Xb = X[b].to(dtype)
        mag = omodel.abs_of_real_complex(Xb)
        m = omodel.cdae_masks(pb, b, mag, causal, training=True, minima=minima, stats={})
        Ymag = m * mag
        if not wiener:
            Y = omodel.phasemix_sep(Xb, Ymag)
        else:
            Y = ref64.blockwise_wiener(Xb, Ymag) if dtype == F64 else omodel.blockwise_wiener(Xb, Ymag)
        mse = mse + oloss.complex_mse([Y], [Yt[b].to(dtype)]) / nb
        msk = msk + oloss.mask_sum([m]) / nb
        Ys.append(Y)
    sdr, _ = sdr_criterion(inverse_dtype(plan, Ys, n, dtype), y_t, dtype)
    (mse + msk + mcoef * sdr).backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad}
    return float(mse.detach()), float(msk.detach()), float(sdr.detach()), grads, minima


def _reference(plan, sd, batch, model, mcoef):
    key = (batch, model, mcoef)
    if key not in _REF:
        causal, wiener = MODELS[model]
        _, y_t, X, Yt = _coefficients(batch)
        _REF[key] = tuple(step_reference(plan, sd, X, Yt, y_t, causal, wiener, mcoef, dt) for dt in (F64, F32))
    return _REF[key]


def _judge_step(plan, case, grads, losses, r64, r32, record=True):
    """tests/test_ref64_train_gpu.py::_judge_gradients with the third loss term: (bad, loose, tight, worst ratio per class)."""
    l64, g64, minima = r64[:3], r64[3], r64[4]
    l32, g32 = r32[:3], r32[3]
    assert sorted(grads) == sorted(g64) == sorted(g32)
    risk_groups = {k.rsplit(".", 1)[0] for k, v in minima.items() if v < RISK}
    risk_blocks = {g.split(".cdaes.")[0] for g in risk_groups}
    F = [f for (_, f, _) in plan.blocks]

    def at_risk(k):
        if k.split(".")[2].startswith("input_"):
            return k.rsplit(".", 1)[0] in risk_blocks
        return k.rsplit(".", 2)[0] in risk_groups

    rec = {}
    for k, ref in g64.items():
        rms_ref = float(ref.pow(2).mean().sqrt())
        rec[k] = (_class(k), rms_ref, _abs_err(grads[k], ref), _abs_err(g32[k], ref), at_risk(k))
    E, A = {c: [0.0, 0.0] for c in CLASSES}, {c: [0.0, 0.0] for c in CLASSES[11:]}
    for k, (c, rms_ref, _, (c_rms, c_max), risky) in rec.items():
        if risky:
            continue
        if c in A:
            A[c] = [max(A[c][0], c_rms), max(A[c][1], c_max)]
            if F[int(k.split(".")[1])] < 2 or rms_ref <= 1e-6:
                continue
        E[c] = [max(E[c][0], c_rms / rms_ref), max(E[c][1], c_max / rms_ref)]
    assert all(e[0] > 0 and e[1] > 0 for e in E.values()), E
    bad, loose, tight = [], [], set()
    worst = {c: (0.0, "") for c in CLASSES}
    for k, (c, rms_ref, (g_rms, g_max), _, risky) in rec.items():
        a_rms, a_max = A.get(c, (0.0, 0.0))
        allow_rms, allow_max = max(E[c][0] * rms_ref, a_rms), max(E[c][1] * rms_ref, a_max)
        ratio = max(g_rms / allow_rms, g_max / allow_max)
        bound = M[GROUP[c]]
        if not risky and ratio > worst[c][0]:
            worst[c] = (ratio, k)
        if ratio <= bound:
            tight.add(k)
        elif risky and g_rms <= KINK_RTOL * rms_ref + bound * a_rms:
            loose.append(k)
        else:
            bad.append(f"{k}: error rms {g_rms:.3e} max {g_max:.3e} (reference rms {rms_ref:.3e}) = {ratio:.2f} x allowed, near a kink: {risky}")
    print(f"\n[step] {case}: {len(risk_groups)} near-kink groups {sorted(risk_groups)[:6]}, {len(loose)} loose tensors {loose[:4]}")
    for c in CLASSES:
        print(f"  {c:12s} E_rms {E[c][0]:.3e} E_max {E[c][1]:.3e}" + (f" A_rms {A[c][0]:.3e} A_max {A[c][1]:.3e}" if c in A else "")
              + f"  worst e_gpu / allowed {worst[c][0]:.2f} at {worst[c][1]}")
    if losses is not None:
        names = ("mse", "mask", "sdr")
        e_gpu = max(abs(g - r) / abs(r) for g, r in zip(losses, l64))
        e_cpu = max(abs(c - r) / abs(r) for c, r in zip(l32, l64))
        print("  loss: " + "  ".join(f"{nm} {g:.9e} (float64 {r:.9e}, fp32 {c:.9e})" for nm, g, r, c in zip(names, losses, l64, l32))
              + f": e_gpu {e_gpu:.2e} E {e_cpu:.2e}")
        if record:
            _T.record("train/loss", case, {"worst_ratio": e_gpu / e_cpu, "E_rms": e_cpu})
        if e_gpu > M["train/loss"] * e_cpu:
            bad.append(f"loss terms: e_gpu {e_gpu:.3e} = {e_gpu / e_cpu:.2f} x E")
    if record:
        for grp in sorted(set(GROUP.values())):
            w = max((worst[c] for c in CLASSES if GROUP[c] == grp), key=lambda t: t[0])
            _T.record(grp, case, {"worst_ratio": w[0], "worst_at": w[1], "loose": len(loose)})
    return bad, loose, tight, worst


STEP_CASES = [("S3", "offline+wiener", 1.0), ("S3", "causal+mixphase", 1.0), ("A", "offline+wiener", 0.1)]


def _step(batch, model, mcoef):
    """(losses, gradients) of one step without the update; mcoef None: ``Trainer()`` as it is built today."""
    key = (batch, model, mcoef)
    if key not in _CASE:
        x, y_t, _, _ = _coefficients(batch)
        tr = _trainer(model) if mcoef is None else _trainer(model, sdr_mcoef=mcoef)
        before = tr.state_dict()
        losses = tr.step(x, y_t, apply_update=False)
        grads = tr.gradients()
        after = tr.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)
        _CASE[key] = (losses, grads)
    return _CASE[key]


@pytest.mark.parametrize("batch,model,mcoef", STEP_CASES)
def test_step_with_the_sdr_term_is_at_fp32_rounding_of_float64(oracle_plan, seeded_sd, batch, model, mcoef):
    r64, r32 = _reference(oracle_plan, seeded_sd, batch, model, mcoef)
    losses, grads = _step(batch, model, mcoef)
    assert len(losses) == 4
    loss, mse, msk, sdr = losses
    assert abs(loss - (mse + msk + mcoef * sdr)) <= 1e-12 * abs(loss)
    bad, loose, tight, _ = _judge_step(oracle_plan, f"{batch} {model} mcoef {mcoef}", grads, (mse, msk, sdr), r64, r32)
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:40])
    assert len(loose) <= LOOSE_SHARE * (len(loose) + len(tight)), (len(loose), loose[:8])


# ---- 4. negative control ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,model,mcoef", STEP_CASES)
def test_a_step_without_the_term_fails_the_bound_in_every_class(oracle_plan, seeded_sd, batch, model, mcoef):
    """The SDR term's share of every gradient class is far above the bound (its RMS is 0.16 .. 13 times the other two terms' in
    the median over blocks at S3): a step that leaves it out -- or scales it wrongly -- cannot pass."""
    r64, r32 = _reference(oracle_plan, seeded_sd, batch, model, mcoef)
    losses, grads = _step(batch, model, None)
    assert len(losses) == 3
    _, _, _, worst = _judge_step(oracle_plan, f"{batch} {model} term off vs mcoef {mcoef}", grads, None, r64, r32, record=False)
    for c in CLASSES:
        assert worst[c][0] > M[GROUP[c]], f"the step without the term passes the bound of {c} ({worst[c][0]:.1f} <= {M[GROUP[c]]})"


# ---- 5. off switch and validation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcoef", [-1.0, 0.0])
def test_term_off_is_bitwise_the_step_without_it(mcoef):
    losses0, grads0 = _step("A", "offline+wiener", None)
    losses, grads = _step("A", "offline+wiener", mcoef)
    assert len(losses) == 3 and tuple(losses) == tuple(losses0)
    assert sorted(grads) == sorted(grads0) and all(torch.equal(grads[k], grads0[k]) for k in grads0)


def test_step_arena_refuses_the_term():
    from xumx_slicq_amd import _lib
    tr = _trainer("offline+wiener", sdr_mcoef=1.0)
    with pytest.raises(_lib.XsqError):
        tr.step_arena(torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda"), 1, 3)


def test_validation_step_with_the_sdr_term_matches_float64(oracle_plan, seeded_sd):
    from xumx_slicq_amd.loss import validation_step
    x, y_t, X, Yt = _coefficients("S3")
    sep = _sep(False)
    got = validation_step(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), x.cuda(), y_t.cuda(), sdr_mcoef=1.0)
    off = validation_step(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), x.cuda(), y_t.cuda())
    assert len(got) == 4 and len(off) == 3 and tuple(got[1:3]) == tuple(off[1:])
    assert abs(got[0] - (got[1] + got[2] + got[3])) <= 1e-12 * abs(got[0])
    refs = []
    with torch.no_grad():
        for dt in (F64, F32):
            if dt == F64:
                Ys, masks = ref64.unmix(seeded_sd, X, False, True)
            else:
                Ys, masks = omodel.unmix(seeded_sd, X, False, True)
            per = ref64.block_losses(Ys, Yt, masks, dtype=dt).mean(0)
            sdr, _ = sdr_criterion(inverse_dtype(oracle_plan, Ys, x.shape[-1], dt), y_t, dt)
            refs.append((float(per[0]), float(per[1]), float(sdr)))
    r64, r32 = refs
    e_gpu = max(abs(g - r) / abs(r) for g, r in zip(got[1:], r64))
    e_cpu = max(abs(c - r) / abs(r) for c, r in zip(r32, r64))
    print(f"[validation] S3 offline+wiener: got {got[1:]}, float64 {r64}, fp32 {r32}: e_gpu {e_gpu:.2e} E {e_cpu:.2e}")
    _T.record("validation", "S3 offline+wiener", {"worst_ratio": e_gpu / e_cpu, "E_rms": e_cpu})
    assert e_gpu <= M["validation"] * e_cpu
