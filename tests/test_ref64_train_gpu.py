"""The training step (xsq_train_step) at fp32 rounding of the float64 reference (oracle/ref64.py): every gradient tensor element by
element, both loss terms, every BatchNorm running statistic, every AdamW update and moment.

Metric and rule are the ones of tests/test_ref64_gpu.py: ``ref64.rel_err`` per tensor; e_gpu = the kernels against ref64, e_cpu = the
fp32 CPU oracle's autograd ON THE SAME COEFFICIENTS (the GPU's own sliCQT output, so only the model, the post-filter, the loss and
their backward are under test) against ref64; assert  e_gpu <= M * E  for every tensor, E = the largest e_cpu over the tensors of
the same class (the thirteen suffixes of CLASSES).  M per class group, by the rule of oracle/parity.py.

Ill-conditioned whitening tensors.  With ONE frequency bin the whitening is an affine map in front of a batch-statistics BatchNorm:
the loss is invariant to it and the gradient is pure cancellation (float64 RMS 1e-12 .. 2e-8).  For input_mean / input_scale the
allowed error of tensor k is therefore  M * max(E_rel * rms(ref_k), A):  E_rel the worst relative e_cpu over blocks with F >= 2 whose
float64 gradient RMS is above 1e-6, A the worst ABSOLUTE error of the fp32 oracle over the tensors of the class on that input.

ReLU kinks.  A tensor may exceed its tight bound only if ref64's smallest |BatchNorm output| in its (block, target) group -- for the
whitening tensors, in any target of its block -- is below RISK: another summation order may land on the other side, which is a
subgradient choice.  It must then stay within 15 % in the RMS metric (the norm-type bound tests/test_training.py puts on every tensor
of such a group), such tensors may number at most 2 % per case, and over the cases of one model every tensor has to be tight at
least once.  No elementwise bound is put on a loose tensor: a unit that switches adds or removes the whole product (gradient x
activation) of one position in every weight element it touches, and an element that sums few positions can move by more than the
tensor's RMS (block 36 / target 0, `6.weight`, offline model on batch A: one element off by 1.09 RMS of the tensor, 3.2 % in RMS).
Tensors of such groups are left out of E (an oracle that flipped would widen it).
"""
import pytest
import torch

from oracle import ref64
from oracle.parity import M_CAP, Tables
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu
RISK, KINK_RTOL, LOOSE_SHARE = 3e-6, 0.15, 0.02
CLASSES = ("0.weight", "1.weight", "1.bias", "3.weight", "4.weight", "4.bias", "6.weight", "7.weight", "7.bias", "9.weight", "9.bias",
           "input_mean", "input_scale")
GROUP = {c: ("train/whiten" if c.startswith("input_") else "train/bn" if c[0] in "147" else "train/conv") for c in CLASSES}

# class group -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_train_parity.json)
M = {
    "train/conv": 4,               # 1.93  (B = 1, S = 3, offline + Wiener: block 52 / target 1, 3.weight); 1.68 on the bf16x6 arm
    "train/bn": 4,                 # 1.90  (same case: block 52 / target 1, 1.weight)
    "train/whiten": 8,             # 2.88  (batch A, causal + Wiener: block 0, input_scale)
    "train/loss": 8,               # 2.97  (batch A, causal + mix-phase, bf16x6; E is two scalars per case: 1.6e-8 .. 6.4e-8)
    "train/bn_running": 4,         # 1.23  (batch A, offline: block 27 / target 3, layer 1)
    "train/adamw": 8,              # 3.12  (defaults, exp_avg of block 47's input_scale: one element, E is its own rounding)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())

_T = Tables("ref64_train_parity", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


def _class(k):
    return next(c for c in CLASSES if k.endswith(c))


# ---- inputs, references (computed once per (batch, model)) ---------------------------------------------------------------
BATCHES = {"A": (2, 44100, 600), "B": (2, 44100, 610), "S3": (1, 9031, 620), "S9": (3, 70000, 630), "S18": (2, 150000, 640)}
MODELS = {"offline+wiener": (False, True), "causal+mixphase": (True, False), "offline+mixphase": (False, False), "causal+wiener": (True, True)}
_SEPS, _COEF, _REF, _CASE = {}, {}, {}, {}


def _inputs(batch):
    B, n, seed0 = BATCHES[batch]
    y_t = torch.stack([0.5 * synth_audio(n, seed=seed0 + j, nb_samples=B) for j in range(4)])
    if batch == "S18":
        y_t[:, 1] *= 40.0                    # row 1 forty times louder: the Wiener window maximum is shared over the batch
    return y_t.sum(0), y_t


def _sep(causal):
    if causal not in _SEPS:
        from xumx_slicq_amd.separator import seeded_separator
        _SEPS[causal] = seeded_separator(realtime=causal)
    return _SEPS[causal]


def _coefficients(batch):
    """(x, y_t, X, Yt): the batch and the GPU's own fp32 coefficients of it, lists over blocks on the host."""
    if batch not in _COEF:
        x, y_t = _inputs(batch)
        enc = _sep(False).nsgt
        _COEF[batch] = (x, y_t, [c.cpu() for c in enc(x.cuda())], [c.cpu() for c in enc(y_t.cuda())])
    return _COEF[batch]


def _reference(plan, sd, batch, model):
    key = (batch, model)
    if key not in _REF:
        causal, wiener = MODELS[model]
        _, _, X, Yt = _coefficients(batch)
        r64 = ref64.training_gradients(plan, sd, X, Yt, causal, wiener)
        r32 = ref64.training_gradients(plan, sd, X, Yt, causal, wiener, dtype=torch.float32)
        _REF[key] = (r64, r32)
    return _REF[key]


def _trainer(model, precision="fp32", **kw):
    from xumx_slicq_amd.training import Trainer
    causal, wiener = MODELS[model]
    sep = _sep(causal)
    tr = Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), precision=precision, **kw)
    tr.wiener = wiener                       # before the first step: the workspace size is cached per (B, S)
    return tr


# ---- the judge of one step's gradients -----------------------------------------------------------------------------------
def _abs_err(got, ref):
    d = got.detach().to("cpu", torch.float64) - ref
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


def _judge_gradients(plan, case, grads, mse, msk, r64, r32, arm="fp32"):
    """Returns (bad, loose, tight, worst ratio per class over the tensors outside the near-kink groups)."""
    mse64, msk64, g64, minima, _ = r64
    mse32, msk32, g32, _, _ = r32
    assert sorted(grads) == sorted(g64) == sorted(g32)
    risk_groups = {k.rsplit(".", 1)[0] for k, v in minima.items() if v < RISK}                  # "sliced_umx.<b>.cdaes.<t>"
    risk_blocks = {g.split(".cdaes.")[0] for g in risk_groups}
    F = [f for (_, f, _) in plan.blocks]

    def at_risk(k):
        if k.split(".")[2].startswith("input_"):
            return k.rsplit(".", 1)[0] in risk_blocks
        return k.rsplit(".", 2)[0] in risk_groups

    rec = {}
    for k, ref in g64.items():
        c = _class(k)
        rms_ref = float(ref.pow(2).mean().sqrt())
        rec[k] = (c, rms_ref, float(ref.abs().max()), _abs_err(grads[k], ref), _abs_err(g32[k], ref), at_risk(k))
    # E per class from the fp32 oracle, near-kink groups left out
    E, A = {c: [0.0, 0.0] for c in CLASSES}, {c: [0.0, 0.0] for c in CLASSES[11:]}
    for k, (c, rms_ref, _, _, (c_rms, c_max), risky) in rec.items():
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
    for k, (c, rms_ref, max_ref, (g_rms, g_max), _, risky) in rec.items():
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
    print(f"\n[train] {case}: {len(risk_groups)} near-kink groups {sorted(risk_groups)[:6]}, {len(loose)} loose tensors {loose[:4]}")
    for c in CLASSES:
        print(f"  {c:12s} E_rms {E[c][0]:.3e} E_max {E[c][1]:.3e}" + (f" A_rms {A[c][0]:.3e} A_max {A[c][1]:.3e}" if c in A else "")
              + f"  worst e_gpu / allowed {worst[c][0]:.2f} at {worst[c][1]}")
    for grp in sorted(set(GROUP.values())):
        w = max((worst[c] for c in CLASSES if GROUP[c] == grp), key=lambda t: t[0])
        _T.record(grp, case, {"M_key": grp if arm in ("fp32", "bf16x6") else f"{grp}/{arm}", "worst_ratio": w[0], "worst_at": w[1], "loose": len(loose),
                              "per_class": {c: {"E_rms": E[c][0], "E_max": E[c][1], "worst_ratio": worst[c][0], "worst_at": worst[c][1]}
                                            for c in CLASSES if GROUP[c] == grp}})
    # loss terms, relative to ref64 (the fp32 oracle's own distance is the scale)
    e_gpu = max(abs(mse - mse64) / mse64, abs(msk - msk64) / msk64)
    e_cpu = max(abs(mse32 - mse64) / mse64, abs(msk32 - msk64) / msk64)
    print(f"  loss: mse {mse:.9e} (float64 {mse64:.9e}, fp32 oracle {mse32:.9e}) mask {msk:.9e} ({msk64:.9e}, {msk32:.9e}): e_gpu {e_gpu:.2e} E {e_cpu:.2e}")
    _T.record("train/loss", case, {"M_key": "train/loss" if arm in ("fp32", "bf16x6") else f"train/loss/{arm}", "worst_ratio": e_gpu / e_cpu, "E_rms": e_cpu})
    if e_gpu > M["train/loss"] * e_cpu:
        bad.append(f"loss terms: e_gpu {e_gpu:.3e} = {e_gpu / e_cpu:.2f} x E")
    return bad, loose, tight, worst


def _case(plan, sd, batch, model, precision="fp32"):
    key = (batch, model, precision)
    if key not in _CASE:
        x, y_t, _, _ = _coefficients(batch)
        r64, r32 = _reference(plan, sd, batch, model)
        tr = _trainer(model, precision)
        before = tr.state_dict()
        _, mse, msk = tr.step(x, y_t, apply_update=False)
        grads = tr.gradients()
        after = tr.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)
        _CASE[key] = _judge_gradients(plan, f"{batch} {model} {precision}", grads, mse, msk, r64, r32, arm=precision)
    return _CASE[key]


def _assert_case(res):
    bad, loose, tight, _ = res
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:40])
    assert len(loose) <= LOOSE_SHARE * (len(loose) + len(tight)), (len(loose), loose[:8])


# ---- gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("batch", ["A", "B"])
def test_every_gradient_is_at_fp32_rounding_of_float64(oracle_plan, seeded_sd, batch, model):
    """B = 2, n = 44,100 (S = 6), the batches of fixtures A and B, all four (first layer, post-filter) combinations: the mask
    backward and the Wiener-EM backward each against both layer-1 types, every tensor element by element."""
    _assert_case(_case(oracle_plan, seeded_sd, batch, model))


@pytest.mark.parametrize("model", ["offline+wiener", "causal+mixphase"])
@pytest.mark.parametrize("batch", ["S3", "S9"])
def test_gradients_at_the_smallest_and_at_an_odd_shape(oracle_plan, seeded_sd, batch, model):
    """B = 1, n = 9,031 (S = 3, the minimum the step accepts: batch statistics over 5 / 2 positions per row, 6 / 3 causal, tiles mostly
    padding) and B = 3, n = 70,000 (S = 9: odd batch, ragged last tiles of the weight-gradient K loop)."""
    _assert_case(_case(oracle_plan, seeded_sd, batch, model))


def test_gradients_across_two_wiener_windows(oracle_plan, seeded_sd):
    """B = 2, n = 150,000 (S = 18), row 1 forty times louder: blocks with T >= 280 have a full 5000-frame window followed by a short
    one in the BACKWARD of the Wiener-EM filter, with the window maximum shared over the batch."""
    assert any(18 * T > 5000 and (18 * T) % 5000 for (_, F, T) in oracle_plan.blocks)
    assert _coefficients("S18")[2][0].shape[3] == 18
    _assert_case(_case(oracle_plan, seeded_sd, "S18", "offline+wiener"))


@pytest.mark.parametrize("model", ["offline+wiener", "causal+mixphase"])
def test_gradients_bf16x6(oracle_plan, seeded_sd, model):
    """The bf16x6 matrix path (exact three-way operand cut) under the same bounds and the same cap."""
    _assert_case(_case(oracle_plan, seeded_sd, "A", model, "bf16x6"))


def test_bf16_arm_fails_the_fp32_bound_in_every_class(oracle_plan, seeded_sd):
    """Trainer(precision="bf16") (the reference's autocast arithmetic: operands rounded to bf16) measured on the same tables: it
    must FAIL the bound the fp32 arm is held to, class by class -- the test resolves that loss of arithmetic."""
    _, _, _, worst = _case(oracle_plan, seeded_sd, "A", "offline+wiener", "bf16")
    for c in CLASSES:
        assert worst[c][0] > M[GROUP[c]], f"bf16 passes the fp32 bound of {c} ({worst[c][0]:.1f} <= {M[GROUP[c]]})"


@pytest.mark.parametrize("model", list(MODELS))
def test_every_tensor_is_tight_in_at_least_one_case(oracle_plan, seeded_sd, model):
    """The near-kink groups of batch A and of batch B must not leave a tensor loose in both."""
    a, b = (_case(oracle_plan, seeded_sd, batch, model) for batch in ("A", "B"))
    _assert_case(a), _assert_case(b)
    never = sorted(set(a[1]) & set(b[1]))
    assert not never, never


# ---- BatchNorm running statistics --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["offline+wiener", "causal+mixphase"])
def test_every_running_statistic_is_at_fp32_rounding_of_float64(oracle_plan, seeded_sd, model):
    """One step with the update on batch A: all 840 running_mean and running_var against ref64.bn_running of ref64's batch
    statistics; E from F.batch_norm(training=True) in fp32 on the CPU (the fp32 oracle's forward); per layer and kind."""
    x, y_t, _, _ = _coefficients("A")
    r64, r32 = _reference(oracle_plan, seeded_sd, "A", model)
    tr = _trainer(model)
    tr.step(x, y_t, apply_update=True)
    got = tr.state_dict()
    assert len(r64[4]) == 840
    labels = [f"layer {l} {kind}" for l in (1, 4, 7) for kind in ("running_mean", "running_var")]
    e_gpu, e_cpu = {l: [] for l in labels}, {l: [] for l in labels}
    for key, (mean, var, count, _, _) in r64[4].items():
        want = ref64.bn_running(seeded_sd[key + ".running_mean"], seeded_sd[key + ".running_var"], mean, var, count)
        cpu = r32[4][key][3:5]
        for kind, w, c in zip(("running_mean", "running_var"), want, cpu):
            lab = f"layer {key.rsplit('.', 1)[1]} {kind}"
            e_gpu[lab].append((key, *(float(v) for v in ref64.rel_err(got[f"{key}.{kind}"], w))))
            e_cpu[lab].append(tuple(float(v) for v in ref64.rel_err(c, w)))
    bad, worst = [], (0.0, "")
    for lab in labels:
        E_rms, E_max = max(e[0] for e in e_cpu[lab]), max(e[1] for e in e_cpu[lab])
        ratios = [(max(r / E_rms, m / E_max), key) for key, r, m in e_gpu[lab]]
        w = max(ratios)
        worst = max(worst, w)
        print(f"[train/bn_running] {model} {lab}: E_rms {E_rms:.3e} E_max {E_max:.3e}; worst e_gpu / E = {w[0]:.2f} at {w[1]} ({len(ratios)} tensors)")
        bad += [f"{key} {lab}: {r:.2f} x E" for r, key in ratios if r > M["train/bn_running"]]
    _T.record("train/bn_running", f"A {model}", {"worst_ratio": worst[0], "worst_at": worst[1]})
    assert not bad, "\n".join(bad[:40])


# ---- AdamW -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,wd", [(1e-2, 0.1), (1e-3, 1e-5)])
def test_every_adamw_update_and_moment_is_at_fp32_rounding_of_float64(oracle_plan, seeded_sd, lr, wd):
    """Three consecutive steps on batch A (offline model).  lr = 1e-2, weight_decay = 0.1 makes the decay 1 - 1e-3 per step, visible
    in fp32 (with the defaults it is 1 - 1e-8, below fp32 resolution).  After every step: the reference is ref64.adamw_step fed the
    GPU's OWN fp32 gradients of that step and the previous float64 state, so only the update kernel is judged; compared on the
    parameter UPDATE p_after - p_before, on exp_avg and on exp_avg_sq, per class, for every trainable tensor; E from
    torch.optim.AdamW(foreach=False) in fp32 on the CPU with the same gradients."""
    x, y_t, _, _ = _coefficients("A")
    tr = _trainer("offline+wiener", lr=lr, weight_decay=wd) if (lr, wd) != (1e-3, 1e-5) else _trainer("offline+wiener")
    assert (tr.lr, tr.weight_decay) == (lr, wd)
    p_gpu = tr.state_dict()
    keys = [k for k in p_gpu if not k.endswith(("running_mean", "running_var"))]       # torch.optim.AdamW's numbering
    p64 = {k: p_gpu[k].double() for k in keys}
    m64 = {k: torch.zeros_like(p64[k]) for k in keys}
    v64 = {k: torch.zeros_like(p64[k]) for k in keys}
    cpu_p = [torch.nn.Parameter(p_gpu[k].clone()) for k in keys]
    opt = torch.optim.AdamW(cpu_p, lr=lr, weight_decay=wd, foreach=False)
    bad, worst = [], {q: (0.0, "") for q in ("update", "exp_avg", "exp_avg_sq")}
    for step in (1, 2, 3):
        tr.step(x, y_t, apply_update=True)
        grads, p_new, st = tr.gradients(), tr.state_dict(), tr.optimizer_state_dict()["state"]
        assert float(st[0]["step"]) == step
        cpu_before = [p.detach().clone() for p in cpu_p]
        for p, k in zip(cpu_p, keys):
            p.grad = grads[k].clone()
        opt.step()
        e_gpu, e_cpu = {}, {}
        for i, k in enumerate(keys):
            pn, mn, vn = ref64.adamw_step(p64[k], grads[k], m64[k], v64[k], step, lr, wd)
            ref = {"update": pn - p64[k], "exp_avg": mn, "exp_avg_sq": vn}
            gpu = {"update": p_new[k].double() - p_gpu[k].double(), "exp_avg": st[i]["exp_avg"], "exp_avg_sq": st[i]["exp_avg_sq"]}
            cs = opt.state[cpu_p[i]]
            cpu = {"update": cpu_p[i].detach().double() - cpu_before[i].double(), "exp_avg": cs["exp_avg"], "exp_avg_sq": cs["exp_avg_sq"]}
            for q, r in ref.items():
                if not bool(r.any()):                                    # a gradient that is exactly zero: so are its moments
                    assert not bool(gpu[q].any()), (k, q)
                    continue
                e_gpu[k, q] = tuple(float(v) for v in ref64.rel_err(gpu[q], r))
                e_cpu[k, q] = tuple(float(v) for v in ref64.rel_err(cpu[q], r))
            p64[k], m64[k], v64[k] = pn, mn, vn
        p_gpu = p_new
        for q in worst:
            for c in CLASSES:
                sel = [k for k in keys if k.endswith(c) and (k, q) in e_gpu]
                E_rms, E_max = max(e_cpu[k, q][0] for k in sel), max(e_cpu[k, q][1] for k in sel)
                ratios = [(max(e_gpu[k, q][0] / E_rms, e_gpu[k, q][1] / E_max), k) for k in sel]
                w = max(ratios)
                worst[q] = max(worst[q], w)
                print(f"[train/adamw] lr {lr} wd {wd} step {step} {q:10s} {c:12s} E_rms {E_rms:.3e} E_max {E_max:.3e} worst e_gpu {max(e_gpu[k, q][0] for k in sel):.3e}"
                      f" = {w[0]:.2f} x E at {w[1]}")
                bad += [f"step {step} {q} {k}: {r:.2f} x E" for r, k in ratios if r > M["train/adamw"]]
    for q, w in worst.items():
        _T.record("train/adamw", f"lr {lr} wd {wd} {q}", {"worst_ratio": w[0], "worst_at": w[1]})
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:40])
