"""The float64 reference of the TRAINING step (oracle/ref64.py: block_gradients, training_gradients, adamw_step, bn_running)
has to be trusted before a kernel is judged by it.  CPU only.

1. ref64.training_gradients against the reference's own autograd (tests/golden/training_step.npz, training_step_b.npz) at the
   tolerances the fp32 oracle is held to, same loose sets.
2. Independent of autograd: central differences of the float64 block loss along seeded random directions.
3. The fp32 oracle's autograd sits at fp32 rounding of it, per tensor class (figures measured on the CPU, factor 4 of headroom).
4. adamw_step against torch.optim.AdamW in float64, bn_running against F.batch_norm(training=True) in float64.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import loss as oloss
from oracle import ref64
from oracle import slicqt as oslicqt
from test_training import KINKS, _check, _inputs, _inputs_b, _loose_b

HEADROOM = 4.0
CLASSES = ("0.weight", "1.weight", "1.bias", "3.weight", "4.weight", "4.bias", "6.weight", "7.weight", "7.bias", "9.weight", "9.bias",
           "input_mean", "input_scale")
MODELS = {"realtime": (True, False), "offline": (False, True)}            # tag -> (causal, wiener)


def _class(k):
    return next(c for c in CLASSES if k.endswith(c))


@pytest.fixture(scope="module")
def steps(oracle_plan, seeded_sd):
    """(batch, tag) -> dict: float64 step from the fp32 oracle's coefficients; for batch A the fp32 oracle's autograd too.  Once."""
    out = {}
    for batch, (x, y_t) in (("A", _inputs(int(load_golden("training_step.npz")["n"]))), ("B", _inputs_b(load_golden("training_step_b.npz")))):
        X, Yt = oslicqt.forward(oracle_plan, x), oslicqt.forward(oracle_plan, y_t)
        for tag, (causal, wiener) in MODELS.items():
            mse, msk, grads, minima, stats = ref64.training_gradients(oracle_plan, seeded_sd, X, Yt, causal, wiener)
            rec = {"mse": mse, "msk": msk, "grads": grads, "minima": minima, "stats": stats, "X": X, "Yt": Yt}
            if batch == "A":
                rec["fp32"] = oloss.training_gradients(oracle_plan, seeded_sd, x, y_t, causal=causal, wiener=wiener)
            out[batch, tag] = rec
    return out


# ---- 1. the reference's own autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["realtime", "offline"])
def test_ref64_training_gradients_match_reference(steps, tag):
    r = steps["A", tag]
    assert all(g.dtype == torch.float64 for g in r["grads"].values())
    _check(load_golden("training_step.npz"), tag, r["mse"], r["msk"], r["grads"], rtol=2e-3)


@pytest.mark.parametrize("tag", ["realtime", "offline"])
def test_ref64_training_gradients_match_reference_fixture_b(steps, tag):
    g = load_golden("training_step_b.npz")
    r = steps["B", tag]
    _check(g, tag, r["mse"], r["msk"], r["grads"], rtol=2e-3, kink_rtol=0.15, loose=_loose_b(g, tag))


def test_ref64_sees_the_kinks_of_fixture_a(steps):
    """The (block, target) groups tests/test_training.py treats loosely are the ones ref64's minima put within 3e-6 of a kink."""
    for tag in MODELS:
        b, t, layer, _ = KINKS[tag]
        key = f"sliced_umx.{b}.cdaes.{t}.{(1, 4, 7)[layer - 1]}"
        assert steps["A", tag]["minima"][key] < 3e-6, (tag, key, steps["A", tag]["minima"][key])


# ---- 2. finite differences ---------------------------------------------------------------------------------------------
FD_STEPS = (1e-6, 5e-7, 2.5e-7, 1.25e-7)      # relative to each tensor's RMS; the first whose quotient agrees with that of half the step
FD_BOUND = 1e-5        # |difference quotient - directional derivative| / |quotient|: 200 times below 2e-3
FD_OWN = FD_BOUND / 100


@pytest.mark.parametrize("tag", ["realtime", "offline"])
def test_block_gradients_equal_central_differences(oracle_plan, seeded_sd, steps, tag):
    """Three blocks (the first with F = 1, block 1 with F = 86, the first with 2 <= F < 20), two seeded directions each over ALL
    trainable tensors of the block (each scaled to its own RMS).  The difference quotient's own error (truncation + rounding) is
    estimated from two steps, |D(h) - D(h/2)| / |D(h/2)|, taken whole: the loss is only piecewise smooth -- every ReLU the step
    crosses bends it -- so the error is no clean h^2 term to extrapolate.  It has to be 100 times below the bound, and the bound is
    200 times below the 2e-3 the gradients are held to against the reference's autograd.  The step is chosen by that estimate alone,
    never by the derivative under test: from h = 1e-5 upwards the quotients of block 1 move by 1e-5 .. 1e-3 between steps (kinks
    crossed), from 1e-7 downwards the rounding of the loss (1e-16 L / h) reaches 1e-7; at 1e-6 two steps agree to 1e-8 -- unless
    a unit sits closer to its kink than the step moves it (offline model, block 2, direction 1: a layer-3 output at 4.5e-6 is
    crossed between 5e-7 and 7e-7 and bends the quotient by 1.6e-3), then the next smaller step of FD_STEPS is taken."""
    causal, wiener = MODELS[tag]
    r = steps["A", tag]
    F = [f for (_, f, _) in oracle_plan.blocks]
    blocks = [F.index(1), 1, next(i for i, f in enumerate(F) if 2 <= f < 20)]
    assert F[1] == 86
    nb = len(F)
    for b in blocks:
        pre = f"sliced_umx.{b}."
        base = {k: v.double() for k, v in seeded_sd.items() if k.startswith(pre) and v.is_floating_point()}
        keys = [k for k in base if k.endswith(oloss.TRAINABLE_SUFFIXES)]

        def loss(shift, d):
            p = dict(base)
            for k in keys:
                p[k] = base[k] + shift * d[k]
            a, c, _, _, _ = ref64.block_gradients(seeded_sd, b, r["X"][b], r["Yt"][b], causal, wiener, nb, params=p)
            return a + c

        for seed in (0, 1):
            gen = torch.Generator().manual_seed(1000 * b + seed)
            d = {k: torch.randn(base[k].shape, generator=gen, dtype=torch.float64) * base[k].pow(2).mean().sqrt() for k in keys}
            want = sum(float((r["grads"][k] * d[k]).sum()) for k in keys)
            for h in FD_STEPS:
                D1 = (loss(h, d) - loss(-h, d)) / (2 * h)
                D2 = (loss(h / 2, d) - loss(-h / 2, d)) / h
                own = abs(D1 - D2) / abs(D2)
                if own <= FD_OWN:
                    break
            err = abs(D2 - want) / abs(D2)
            print(f"{tag} block {b} (F {F[b]}) direction {seed}: h {h:.2e} derivative {want:.9e}, quotient {D2:.9e}, error {err:.2e}, own error {own:.2e}")
            assert own <= FD_OWN, (tag, b, seed, own)
            assert err <= FD_BOUND, (tag, b, seed, err)


# ---- 3. the fp32 oracle sits at fp32 rounding of ref64 -------------------------------------------------------------------
# measured on the CPU on fixture A's batch: worst relative RMS / max over the 3,080 conv, BatchNorm and layer-4 bias tensors;
# worst over the whitening tensors of blocks with F >= 2 (float64 gradient RMS above 1e-6); worst ABSOLUTE RMS error over all 70
# input_mean / input_scale (with one frequency bin the loss is invariant to the whitening: those gradients are cancellation)
MEASURED = {"offline": dict(rms=2.71e-6, mx=3.1e-5, whiten=7.4e-6, abs_mean=3.4e-10, abs_scale=7.2e-10),
            "realtime": dict(rms=2.53e-6, mx=2.7e-5, whiten=8.6e-6, abs_mean=9.0e-10, abs_scale=6.4e-9)}


@pytest.mark.parametrize("tag", ["realtime", "offline"])
def test_fp32_oracle_gradients_are_at_rounding_per_class(oracle_plan, steps, tag):
    r, want = steps["A", tag], MEASURED[tag]
    _, mse, msk, g32 = r["fp32"]
    assert abs(mse - r["mse"]) < 1e-6 * r["mse"] and abs(msk - r["msk"]) < 1e-6 * r["msk"]
    assert sorted(g32) == sorted(r["grads"])
    worst = {c: [0.0, 0.0] for c in CLASSES}
    absw = {"input_mean": 0.0, "input_scale": 0.0}
    past = []
    for k, ref in r["grads"].items():
        c = _class(k)
        d = g32[k].double() - ref
        if c in absw:
            absw[c] = max(absw[c], float(d.pow(2).mean().sqrt()))
            b = int(k.split(".")[1])
            if oracle_plan.blocks[b][1] < 2 or float(ref.pow(2).mean().sqrt()) <= 1e-6:
                continue
        e_rms, e_max = (float(v) for v in ref64.rel_err(g32[k], ref))
        worst[c] = [max(worst[c][0], e_rms), max(worst[c][1], e_max)]
        if c not in absw and e_rms > 1e-4:
            past.append(k)
    for c in CLASSES:
        print(f"{tag} {c:12s} worst rel_rms {worst[c][0]:.2e} rel_max {worst[c][1]:.2e}")
    print(f"{tag} absolute RMS error, all 70: input_mean {absw['input_mean']:.2e} input_scale {absw['input_scale']:.2e}")
    assert not past, past
    for c in CLASSES[:11]:
        assert worst[c][0] < HEADROOM * want["rms"] and worst[c][1] < HEADROOM * want["mx"], (c, worst[c])
    for c in CLASSES[11:]:
        assert 0 < worst[c][0] < HEADROOM * want["whiten"], (c, worst[c])
    assert absw["input_mean"] < HEADROOM * want["abs_mean"] and absw["input_scale"] < HEADROOM * want["abs_scale"], absw


# ---- 4. the optimiser and the running statistics ---------------------------------------------------------------------------
@pytest.mark.parametrize("lr,wd", [(1e-2, 0.1), (1e-3, 1e-5)])
def test_adamw_step_is_torch_adamw_in_float64(lr, wd):
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(4, 5, 3, generator=gen, dtype=torch.float64)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([par], lr=lr, weight_decay=wd, foreach=False)
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2, 3):
        g = torch.randn(p0.shape, generator=gen, dtype=torch.float64) * 10.0 ** (-3 * step)
        par.grad = g.clone()
        opt.step()
        p, m, v = ref64.adamw_step(p, g, m, v, step, lr, wd)
        st = opt.state[par]
        for got, ref in ((p, par.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert float((got - ref).abs().max()) <= 1e-15 * float(ref.abs().max()), (step, float((got - ref).abs().max()))
    assert float((p - p0).abs().min()) > 0


def test_bn_running_is_batch_norm_in_training_mode(seeded_sd, steps):
    """All 840 BatchNorm layers on fixture A's batch: ref64.bn_running of the recorded batch statistics against the buffers that
    F.batch_norm(training=True) updated in float64 in the same forward."""
    st = steps["A", "offline"]["stats"]
    assert len(st) == 840
    for key, (mean, var, count, rm, rv) in st.items():
        assert rm.dtype == torch.float64 and count > 1
        m, v = ref64.bn_running(seeded_sd[key + ".running_mean"], seeded_sd[key + ".running_var"], mean, var, count)
        assert float((m - rm).abs().max()) <= 1e-14 * float(rm.abs().max()), key
        assert float((v - rv).abs().max()) <= 1e-14 * float(rv.abs().max()), key
        assert float((rm - seeded_sd[key + ".running_mean"].double()).abs().max()) > 0
