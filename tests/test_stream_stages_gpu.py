"""The two transform halves of a streaming step through the C ABI, on both plans, against float64: ``xsq_slicqt_forward_ring`` (the
window's slices read from the audio ring at their absolute index) per band, and ``xsq_slicqt_inverse_masked_carry`` (the new slices
of a step, overlap-added onto the carried half) per stem and per block.  tests/test_stream_gpu.py judges a session through the RMS
of a whole stem, a thousand roundings wide; here one wrong band of a ring-read slice or one block of a carried half is all of its
row's error.  Rule, metric and helper are those of tests/test_ref64_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err``, E the LARGEST
error of the fp32 CPU oracle (``oracle.slicqt.forward`` / ``inverse``) over the members of the stage on the same input, M per stage a
power of two, the smallest that is at least twice the worst e_gpu / E measured on MI355X, at most ``M_CAP``.  The measured tables are
in profiles/stream_stage_parity.json, the worst ratio behind each M in DESIGN.md section 2 (item 11) and 4.11.

The references rest on the slice-shift property that tests/test_stream_cpu.py asserts in float64: the slices f .. f + S - 1 of a
stream are the slices 1 .. S of ``forward`` of the (2S + 2)h samples they cover, wherever those lie in the stream; the blocks a chain
of carried calls emits are ``inverse`` of all the slices.

Every buffer a correct kernel must not read is NaN (ring slots at or after n, the slots of the samples that arrive in x_new, ring
slots outside the window, the window slices around [first, first + S), the first carry_in, carry_out before a call, the padding
between output rows), and what it must not write is compared bit for bit afterwards.

Wall time of the module on MI355X: 5.5 s for its 11 tests, references included (the slowest, the eight ring cases of Mel-32, 1.0 s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import ref64
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables
from test_ref64_mel_cpu import MEL, make_mel_plan, make_mel_sd, one_thread
from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/stream_stage_parity.json).  Both start
# from the 4 of the whole-call default arms ("forward" and "inverse" of tests/test_ref64_gpu.py / test_ref64_mel_gpu.py), which
# run the same arithmetic; a stage that needed more than its whole-call twin would be a finding.
M = {
    "forward_ring": 4,             # 1.47  (Mel-32, first_slice = 0, S = 3, whitened input, band 5, Lg 16); Bark-262: 1.18 (first_slice = 0, xin, band 238)
    "inverse_carry": 4,            # 1.49  (Mel-32, B = 2, stem 2, every partition: they are the same bits); Bark-262: 1.15 (B = 1, stem 1)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())

_T = Tables("stream_stage_parity", M)
_judge = _T.judge
NAN = float("nan")
PLANS = ["bark", "mel"]
FAR_SLICE = {"bark": 600_000, "mel": 5_000_000}          # even; 2 * first_slice * h > 2^32 samples on either plan
PARTITIONS = [(9,), (2, 1, 1, 1, 1, 1, 1, 1), (3, 2, 2, 2), (4, 3, 2), (2, 7)]
S_TOT = 9


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


@pytest.fixture(scope="module")
def rigs(oracle_plan, seeded_sd):
    """plan name -> (oracle plan, engine, per-band whitening tables of the seeded model as fp32 host tensors)."""
    from xumx_slicq_amd.transforms import NSGTBase
    out = {}
    for name in PLANS:
        if name == "bark":
            p, sd, base = oracle_plan, seeded_sd, NSGTBase("bark", 262, 32.9, device="cuda")
        else:
            p = make_mel_plan()
            sd, base = make_mel_sd(p), NSGTBase(*MEL, device="cuda")
        mean = torch.cat([sd[f"sliced_umx.{b}.input_mean"].float().reshape(-1) for b in range(len(p.blocks))])
        scale = torch.cat([sd[f"sliced_umx.{b}.input_scale"].float().reshape(-1) for b in range(len(p.blocks))])
        assert mean.numel() == scale.numel() == p.nbands and base.plan.L == p.L
        out[name] = (p, base.nsgt, mean, scale)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _band_labels(p, rows=None):
    lab = [f"band {j} Lg {int(p.Lg[j])}" for j in range(p.nbands)]
    return lab if rows is None else [f"row {r} {l}" for r in range(rows) for l in lab]


def _real_band_err(got, ref, per_row):
    """``ref64.band_rel_err`` for real (*lead, F, S, T) blocks."""
    rms, mx = [], []
    for a, b in zip(got, ref):
        F = b.shape[-3]
        r, m = ref64.rel_err(a.reshape(-1, F, *b.shape[-2:]), b.reshape(-1, F, *b.shape[-2:]), keep=(0, 1) if per_row else (1,))
        rms.append(r)
        mx.append(m)
    return np.concatenate(rms, axis=-1), np.concatenate(mx, axis=-1)


# ======================================================================================================================
# forward from the ring
# ======================================================================================================================
class RingCase:
    """S slices from absolute slice ``first`` on for ``B`` items of two channels, a stream of ``n`` samples so far (``n_off`` samples
    short of the window's end), the last ``count`` of them in x_new with row stride ``count + pad``; ``stale``: what lies in the
    ring slots at or after n besides NaN in row 0."""

    def __init__(self, what, B, first, S, ring, n_off=0, count=0, kind="synth", stale=NAN):
        self.what, self.B, self.first, self.S, self.ring, self.n_off, self.count, self.kind, self.stale = what, B, first, S, ring, n_off, count, kind, stale


def _ring_layout(p, case, v):
    """Host (ring, x_new, ring after the call, n) for the window samples ``v`` (2B, (2S + 2)h), v[:, j] = absolute sample
    (2 first - 2)h + j."""
    h, BC = p.h, 2 * case.B
    base = (2 * case.first - 2) * h
    span = (2 * case.S + 2) * h
    n = base + span - case.n_off
    new0 = n - case.count
    assert v.shape == (BC, span) and case.ring > p.L and span - max(0, -base) <= case.ring and n > max(base, 0)
    assert case.count == 0 or (new0 >= 2 * case.first * h and n <= base + span)
    ring = torch.full((BC, case.ring), NAN)
    after = ring.clone()
    stride = case.count + 29
    x_new = torch.full((BC, stride), NAN)
    j = torch.arange(span)
    absolute = base + j
    slot = absolute % case.ring                                     # (int64; Python's sign convention, unused where absolute < 0)
    old = (absolute >= 0) & (absolute < new0)
    new = (absolute >= new0) & (absolute < n)
    late = absolute >= n
    ring[:, slot[old]] = v[:, old]
    ring[1:, slot[late]] = case.stale                               # row 0 keeps NaN behind n, the others hold `stale`
    after.copy_(ring)
    after[:, slot[new]] = v[:, new]
    if case.count:
        x_new[:, :case.count] = v[:, new]
    vz = v.clone()
    vz[:, (absolute < 0) | late] = 0.0                              # what the transform is to see
    return ring, x_new, after, n, stride, vz


def _run_ring(rig, case, v):
    """(coefficient blocks, whitened blocks, ring after, expected ring after, x_new untouched?, vz) of one call."""
    from xumx_slicq_amd import _lib
    p, eng, mean, scale = rig
    BC, S = 2 * case.B, case.S
    ring, x_new, after, n, stride, vz = _ring_layout(p, case, v)
    dev = torch.device("cuda")
    handle = eng.handle(dev)
    ring_d, new_d = ring.to(dev), x_new.to(dev)
    mean_d, scale_d = mean.to(dev), scale.to(dev)
    coef = torch.full((eng.table.numel(BC, S),), NAN, device=dev)
    xin = torch.full((eng.table.numel(BC, S, complex_=False),), NAN, device=dev)
    nbytes = _lib.lib.xsq_slicqt_forward_workspace(handle, BC, (2 * S - 3) * p.h)          # (that many samples give S slices)
    assert nbytes > 0, _lib.last_error()
    ws = eng.workspace(dev, nbytes)
    _lib.check(_lib.lib.xsq_slicqt_forward_ring(handle, ring_d.data_ptr(), case.ring, BC, case.first, S, n,
                                                new_d.data_ptr() if case.count else None, stride if case.count else 0, case.count,
                                                coef.data_ptr(), xin.data_ptr(), mean_d.data_ptr(), scale_d.data_ptr(), 0,
                                                ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "xsq_slicqt_forward_ring")
    torch.cuda.synchronize()
    lead = (case.B, 2)
    Cg = [c.cpu() for c in eng.table.views(coef, lead, S)]
    Xg = [c.cpu() for c in eng.table.views(xin, lead, S, complex_=False)]
    assert torch.equal(_bits(new_d.cpu()), _bits(x_new)), f"{case.what}: x_new was written"
    return Cg, Xg, ring_d.cpu(), after, vz


def _window_signal(p, case, seed):
    span, B = (2 * case.S + 2) * p.h, case.B
    x = synth_audio(span, seed=seed, nb_samples=B)                  # (B, 2, span): every band above 0.5 RMS
    if case.kind == "scaled":                                       # the right channel and batch row 1 at 1e-3 (tests/test_ref64_gpu.py)
        x[:, 1] *= 1e-3
        if B > 1:
            x[1] *= 1e-3
    return x.reshape(2 * B, span)


def _judge_ring(rig, name, case, Cg, Xg, vz):
    """Slices 1 .. S of the transforms of the (2S + 2)h window samples are the call's slices (tests/test_stream_cpu.py)."""
    p, _, mean, scale = rig
    S, per_row = case.S, case.kind == "scaled"
    lead = (case.B, 2)
    cut = lambda blocks: [b[..., 1:S + 1, :, :] for b in blocks]
    ref = cut(ref64.forward(p, vz.reshape(*lead, -1)))
    with one_thread():
        orc = cut(O.forward(p, vz.reshape(*lead, -1)))
    assert all(c.shape == r.shape for c, r in zip(Cg, ref))
    labels = _band_labels(p, 2 * case.B if per_row else None)
    bad, _ = _judge("forward_ring", f"{name} {case.what} coef", ref64.band_rel_err(Cg, ref, per_row), ref64.band_rel_err(orc, ref, per_row), labels)
    # xin = (|coef| + mean[band]) * scale[band]: float64 from ref64's coefficients, E from the fp32 oracle's in fp32
    off, xr, xo = 0, [], []
    for (j0, F, T), r, o in zip(p.blocks, ref, orc):
        mu, sc = mean[j0:j0 + F].reshape(F, 1, 1), scale[j0:j0 + F].reshape(F, 1, 1)
        xr.append((ref64.abs_of_real_complex(r) + mu.double()) * sc.double())
        xo.append((omodel.abs_of_real_complex(o) + mu) * sc)
        off += F
    assert off == p.nbands and all(a.shape == b.shape for a, b in zip(Xg, xr))
    b2, _ = _judge("forward_ring", f"{name} {case.what} xin", _real_band_err(Xg, xr, per_row), _real_band_err(xo, xr, per_row), labels)
    return [f"{case.what} coef {m}" for m in bad] + [f"{case.what} xin {m}" for m in b2]


def _wrapping_first_slice(p, ring, lo, hi):
    """The smallest even first_slice in [2, 64) whose first sample lies w samples in front of the ring's end with lo < w < hi, w
    odd: the slice wraps between the two samples of one of the kernel's pairs.  None: this ring has none."""
    for f in range(2, 64, 2):
        w = ring - ((2 * f - 2) * p.h) % ring
        if lo < w < hi and w % 2 == 1:
            return f
    return None


def _odd_ring(p):
    """(ring, first_slice that wraps in its first half, first_slice that wraps in its second half) for the shortest odd ring of at
    least 8h + 1 samples that has both: a session's ring is even, so only a direct call can wrap inside a pair."""
    h = p.h
    for ring in range(8 * h + 1, 10 * h, 2):
        # between h and 3h the slice window is above one half: a wrap a few samples into a slice, where the window is all but zero,
        # hides a duplicated sample (measured: a wrap 15 samples in stayed below E)
        f1, f2 = _wrapping_first_slice(p, ring, h, 2 * h), _wrapping_first_slice(p, ring, 2 * h, 3 * h)
        if f1 is not None and f2 is not None:
            for f in (f1, f2):
                w = ring - ((2 * f - 2) * h) % ring
                assert min(float(p.tw[w - 1]), float(p.tw[w])) > 0.5, (ring, f, w)
            return ring, f1, f2
    raise AssertionError("no odd ring with both wraps")


def _ring_cases(p):
    h = p.h
    odd, first_half, second_half = _odd_ring(p)
    assert odd % 2 == 1 and odd >= 8 * h
    session = (2 * (3 + 2 + 2) + 2) * h          # the ring of a causal session at m = 2
    return [
        RingCase("first_slice=0 S=3", 1, 0, 3, odd),
        RingCase(f"wrap in the first half, first_slice={first_half} S=3", 1, first_half, 3, odd),
        RingCase(f"wrap in the second half, first_slice={second_half} S=3 scaled", 2, second_half, 3, odd, kind="scaled"),
        RingCase("n ends inside the last slice, stale 7.0 and NaN behind it, S=3", 1, 4, 3, odd, n_off=h + 123, stale=7.0),
        RingCase("x_new of 1 sample, n inside the last slice, S=6", 2, 4, 6, session, n_off=2 * h + 5, count=1),
        RingCase("x_new of 2h samples S=6 scaled", 2, 5, 6, session, count=2 * h, kind="scaled"),
        RingCase("x_new of an m=2 step (4h samples) S=6", 1, 6, 6, session, count=4 * h),
        RingCase("S=13 BC=4, x_new of 2h - 1 samples", 2, 3, 13, 28 * h + 1, n_off=1, count=2 * h - 1),
    ]


@pytest.mark.parametrize("name", PLANS)
def test_forward_from_the_ring_is_at_fp32_rounding_of_float64_in_every_band(rigs, name):
    """first_slice = 0 (samples before 0 read as zero), a wrap of the ring inside the first and inside the second half of a slice
    (between the two samples of a pair), n ending inside the last slice with stale data behind it, new samples from x_new (1, 2h,
    the 4h of an m = 2 step) with a row stride beyond their count, BC = 2 and 4, S = 3, 6 and 13.  After each call the ring holds
    the new samples and is otherwise unchanged, bit for bit, NaNs included."""
    rig = rigs[name]
    p = rig[0]
    bad = []
    for i, case in enumerate(_ring_cases(p)):
        v = _window_signal(p, case, seed=20261019 + 17 * i + p.L)
        Cg, Xg, ring_after, want_after, vz = _run_ring(rig, case, v)
        same = torch.equal(_bits(ring_after), _bits(want_after))
        print(f"[forward_ring] {name} {case.what}: ring after the call as expected: {same}")
        if not same:
            d = (_bits(ring_after) != _bits(want_after)).nonzero()
            bad.append(f"{case.what}: {d.shape[0]} ring slots differ from the expected, first at (row, slot) {d[0].tolist()}")
        bad += _judge_ring(rig, name, case, Cg, Xg, vz)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", PLANS)
def test_forward_from_the_ring_beyond_2_to_the_32_samples_is_the_same_bits(rigs, name):
    """An even first_slice whose samples lie beyond 2^32 against the same window at first_slice = 8 with the same ring phase (a ring
    of 16h samples: the phase is (first_slice - 1) mod 8 blocks), 2h new samples in x_new: coefficients, whitened input and the
    ring afterwards are the same bits, and the near one is judged against float64."""
    rig = rigs[name]
    p = rig[0]
    h, far = p.h, FAR_SLICE[name]
    assert far % 8 == 0 and 2 * far * h > 2 ** 32
    got = {}
    for first in (8, far):
        case = RingCase(f"first_slice={first} S=6 x_new of 2h", 1, first, 6, 16 * h, count=2 * h)
        assert ((2 * first - 2) * h) % case.ring == 14 * h
        v = _window_signal(p, case, seed=777 + p.L)
        got[first] = (case, *_run_ring(rig, case, v))
    (case, Cn, Xn, ring_n, want_n, vz), (_, Cf, Xf, ring_f, want_f, _) = got[8], got[far]
    assert torch.equal(_bits(want_n), _bits(want_f))
    assert torch.equal(_bits(ring_n), _bits(want_n)), "near: ring after the call"
    assert torch.equal(_bits(ring_f), _bits(want_f)), "far: ring after the call"
    for b, (a, c) in enumerate(zip(Cn, Cf)):
        assert torch.equal(_bits(a), _bits(c)), f"coefficients of block {b} differ between first_slice 8 and {far}"
    for b, (a, c) in enumerate(zip(Xn, Xf)):
        assert torch.equal(_bits(a), _bits(c)), f"whitened input of block {b} differs between first_slice 8 and {far}"
    bad = _judge_ring(rig, name, case, Cn, Xn, vz)
    assert not bad, "\n".join(bad)


# ======================================================================================================================
# carried inverse
# ======================================================================================================================
def _arena(blocks):
    return torch.cat([b.reshape(-1) for b in blocks])


def _window(blocks, a, S, first, S_window, complex_):
    """[a, a + S) of the slice axis at [first, first + S) of a NaN window of S_window slices."""
    ax = -3 if complex_ else -2
    out = []
    for b in blocks:
        shape = list(b.shape)
        shape[ax] = S_window
        w = torch.full(shape, NAN)
        w.narrow(ax, first, S).copy_(b.narrow(ax, a, S))
        out.append(w)
    return _arena(out)


def _run_chain(rig, masks, mix, parts, length, pad=37):
    """The S_TOT slices of ``masks`` (lead (*, 2) blocks (.., F, S, T), BC channels) times ``mix`` (BCx channels) through a chain of
    xsq_slicqt_inverse_masked_carry calls of ``parts`` slices: (BC, length) joined output."""
    from xumx_slicq_amd import _lib
    p, eng = rig[0], rig[1]
    h = p.h
    dev = torch.device("cuda")
    handle = eng.handle(dev)
    BC = int(np.prod(masks[0].shape[:-3]))
    BCx = int(np.prod(mix[0].shape[:-4]))
    assert sum(parts) == S_TOT and masks[0].shape[-2] == mix[0].shape[-3] == S_TOT and BC % BCx == 0
    assert 2 * (S_TOT - 2) * h < length < 2 * (S_TOT - 1) * h, "the length ends inside the last block"
    stride = length + pad
    y = torch.full((BC, stride), NAN, device=dev)
    carry = [torch.full((BC, 2 * h), NAN, device=dev) for _ in range(2)]
    a = col = cur = 0
    for i, S in enumerate(parts):
        shift = 0 if i == 0 else 1
        first, S_window = 1 + i % 2, S + 2 + i % 3                 # slices in front and behind that the call must not take
        mw, xw = _window(masks, a, S, first, S_window, False).to(dev), _window(mix, a, S, first, S_window, True).to(dev)
        n = min((S - 1 + shift) * 2 * h, length - col)
        assert n >= 1
        nbytes = _lib.lib.xsq_slicqt_inverse_carry_workspace(handle, BC, BCx, S)
        assert nbytes > 0, _lib.last_error()
        ws = eng.workspace(dev, nbytes)
        carry[1 - cur].fill_(NAN)
        _lib.check(_lib.lib.xsq_slicqt_inverse_masked_carry(handle, mw.data_ptr(), xw.data_ptr(), BC, BCx, S_window, first, S, shift, n,
                                                            y.data_ptr() + 4 * col, stride, carry[cur].data_ptr(), carry[1 - cur].data_ptr(),
                                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "xsq_slicqt_inverse_masked_carry")
        torch.cuda.synchronize()
        a, col, cur = a + S, col + n, 1 - cur
    assert col == length
    y = y.cpu()
    assert bool(torch.isnan(y[:, length:]).all()), "the padding between the output rows was written"
    return y[:, :length].contiguous()


@pytest.fixture(scope="module")
def carry_inputs(rigs):
    """(plan name, B) -> masks (4, B, 2, F, 9, T) in [0, 1], mix (B, 2, F, 9, T, 2), length, float64 reference (4, B, 2, length) and
    the fp32 oracle's error per stem; computed once, shared by the partitions."""
    cache = {}

    def get(name, B):
        if (name, B) not in cache:
            p = rigs[name][0]
            gen = torch.Generator().manual_seed(100 * B + p.L)
            masks = [torch.rand(4, B, 2, F, S_TOT, T, generator=gen) for (_, F, T) in p.blocks]
            mix = [torch.randn(B, 2, F, S_TOT, T, 2, generator=gen) for (_, F, T) in p.blocks]
            length = 2 * (S_TOT - 1) * p.h - 333
            ref = ref64.inverse(p, [m.double().unsqueeze(-1) * x.double() for m, x in zip(masks, mix)], length)
            e_cpu = ref64.rel_err(O.inverse(p, [m.unsqueeze(-1) * x for m, x in zip(masks, mix)], length), ref, keep=(0,))
            cache[name, B] = (masks, mix, length, ref, e_cpu)
        return cache[name, B]
    return get


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", PLANS)
def test_chains_of_carried_inverses_are_at_fp32_rounding_of_float64_per_stem(rigs, carry_inputs, name, B):
    """Nine slices, BC = 8B mask channels on BCx = 2B mix channels, through the partitions (9), (2, 1 x 7), (3, 2, 2, 2), (4, 3, 2)
    and (2, 7): the first call with shift = 0 and a NaN carry_in, the others on the half their predecessor left, the last clipped
    by a length that ends inside the last block.  Whether the partitions agree bit for bit is printed and recorded, not asserted."""
    masks, mix, length, ref, e_cpu = carry_inputs(name, B)
    bad, outs = [], {}
    for parts in PARTITIONS:
        y = _run_chain(rigs[name], masks, mix, parts, length).reshape(4, B, 2, length)
        outs[parts] = y
        b, _ = _judge("inverse_carry", f"{name} B={B} partition {parts}", ref64.rel_err(y, ref, keep=(0,)), e_cpu, [f"stem {t}" for t in range(4)])
        bad += [f"partition {parts} {m}" for m in b]
    same = {str(parts): bool(torch.equal(_bits(y), _bits(outs[PARTITIONS[0]]))) for parts, y in outs.items()}
    print(f"[inverse_carry] {name} B={B}: partitions bitwise equal to {PARTITIONS[0]}: {same}")
    _T.record("inverse_carry_partitions", f"{name} B={B}", {"M_key": "inverse_carry_partitions (bitwise equal to one call of 9; not judged)",
                                                             "worst_ratio": 0.0, "bitwise": same})
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", PLANS)
def test_chain_of_carried_inverses_of_each_block_alone(rigs, name):
    """Mix coefficients that are zero except in ONE block, one batch item per block (BCx = BC = 2 x 70 / 23 channels, one chain of
    (4, 3, 2)): a wrong dual-window value, or a wrong slice of one block taken out of the window, is all of its item's energy."""
    p = rigs[name][0]
    nb = len(p.blocks)
    gen = torch.Generator().manual_seed(nb)
    masks, mix = [], []
    for k, (_, F, T) in enumerate(p.blocks):
        x = torch.zeros(nb, 2, F, S_TOT, T, 2)
        x[k] = torch.randn(2, F, S_TOT, T, 2, generator=gen)
        mix.append(x)
        masks.append(torch.rand(nb, 2, F, S_TOT, T, generator=gen))
    length = 2 * (S_TOT - 1) * p.h - 333
    ref = ref64.inverse(p, [m.double().unsqueeze(-1) * x.double() for m, x in zip(masks, mix)], length)
    e_cpu = ref64.rel_err(O.inverse(p, [m.unsqueeze(-1) * x for m, x in zip(masks, mix)], length), ref, keep=(0,))
    y = _run_chain(rigs[name], masks, mix, (4, 3, 2), length).reshape(nb, 2, length)
    bad, _ = _judge("inverse_carry", f"{name} one block per item, partition (4, 3, 2)", ref64.rel_err(y, ref, keep=(0,)), e_cpu,
                    [f"block {b} F {F} T {T}" for b, (_, F, T) in enumerate(p.blocks)], full_table=True)
    assert not bad, "\n".join(bad)


def test_stage_entry_points_refuse_what_they_cannot_run(rigs):
    """The argument checks the stage tests lean on: new samples outside the second halves of the call's slices, a window that does
    not fit the ring, slices outside the window arena, shift = 1 without a carry."""
    from xumx_slicq_amd import _lib
    p, eng, mean, scale = rigs["mel"]
    h = p.h
    dev = torch.device("cuda")
    handle = eng.handle(dev)
    buf = torch.zeros(1 << 20, device=dev)         # (large enough for every arena, ring and output these shapes name)
    ws = eng.workspace(dev, 1 << 24)
    ring = lambda *a: _lib.lib.xsq_slicqt_forward_ring(handle, buf.data_ptr(), *a, buf.data_ptr(), None, None, None, 0, ws.data_ptr(), ws.numel(),
                                                        _lib.stream_ptr())
    #         ring_len BC first S n          x_new           stride count
    assert ring(8 * h, 2, 4, 3, 14 * h, buf.data_ptr(), 7 * h, 7 * h) != 0          # new samples reach into the first half of slice 4
    assert ring(8 * h - 1, 2, 4, 3, 14 * h, None, 0, 0) != 0                          # 3 slices span 8h samples
    assert ring(4 * h, 2, 0, 3, 6 * h, None, 0, 0) != 0                               # the ring must be longer than a slice
    assert ring(8 * h, 2, 4, 3, 14 * h, buf.data_ptr(), h - 1, h) != 0                # row stride below the count
    inv = lambda *a: _lib.lib.xsq_slicqt_inverse_masked_carry(handle, buf.data_ptr(), buf.data_ptr(), *a, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    #        BC BCx S_window first S shift length y            stride   carry_in        carry_out
    assert inv(8, 2, 4, 2, 3, 1, 6 * h, buf.data_ptr(), 6 * h, buf.data_ptr(), buf.data_ptr()) != 0      # [2, 5) of a window of 4
    assert inv(8, 2, 4, 1, 3, 1, 6 * h, buf.data_ptr(), 6 * h, None, buf.data_ptr()) != 0                # shift = 1 needs carry_in
    assert inv(8, 2, 4, 1, 1, 0, 1, buf.data_ptr(), 6 * h, None, buf.data_ptr()) != 0                    # one slice at shift 0 closes no block
    assert inv(8, 3, 4, 1, 3, 1, 6 * h, buf.data_ptr(), 6 * h, buf.data_ptr(), buf.data_ptr()) != 0      # 3 mix channels do not divide 8
    assert inv(8, 2, 4, 1, 3, 1, 6 * h + 1, buf.data_ptr(), 7 * h, buf.data_ptr(), buf.data_ptr()) != 0  # three blocks are 6h samples
    torch.cuda.synchronize()
