"""Autograd through the sliCQT on the GPU: the adjoint of the forward transform (xsq_slicqt_forward_adjoint) at fp32 rounding of
float64 autograd through ``oracle.ref64.forward``, ``NSGT_SL`` / ``INSGT_SL`` as differentiable modules, and everything they did
before, bit for bit, with grad mode off.

Rule and metric are those of tests/test_ref64_gpu.py and tests/test_sdr_gpu.py:  e_gpu <= M * E  by ``ref64.rel_err`` per channel
row, E the largest error against float64 of the SAME closed form evaluated in float32 / complex64 on the CPU on the same input
(tests/test_autograd_cpu.py carries it with a dtype), M a power of two <= M_CAP by the rule of DESIGN.md section 2 (smallest power
of two >= twice the worst ratio measured on MI355X).  Shapes are those of tests/test_sdr_gpu.py, for the same reasons."""
import numpy as np
import pytest
import torch

from oracle import ref64
from oracle import slicqt as O
from oracle.parity import M_CAP, Tables
from test_autograd_cpu import F32, F64, autograd_forward_adjoint, forward_adjoint_closed_form, mel_plan, random_cotangents

pytestmark = pytest.mark.gpu

# stage -> M, with the worst e_gpu / E measured on MI355X behind it (profiles/ref64_autograd_parity.json)
M = {
    "fwd_adjoint": 4,              # 1.03  (Bark-262, BC 8, n = 9031: row 7, and BC 3, n = 70000: row 2; 0.89 with the edge bands alone and with one F = 1 block)
    "fwd_adjoint/rocfft": 4,       # 1.17  (Mel-32, BC 8, n = 32768: row 2; 1.05 with the edge bands alone)
    "magnitude_loss": 2,           # 0.82  (Bark-262, B 2, n = 9031: row 3; E is the oracle's fp32 autograd)
}
assert all(m <= M_CAP and m & (m - 1) == 0 for m in M.values())
_T = Tables("ref64_autograd_parity", M)


@pytest.fixture(scope="module", autouse=True)
def _dump_tables():
    yield
    _T.dump()


_ENG = {}


def _setup(which):
    """(oracle plan, NSGTBase, engine) of Bark-262 (hand-written slice FFT) or Mel-32 (rocFFT), made once."""
    if which not in _ENG:
        from xumx_slicq_amd.transforms import NSGTBase
        if which == "bark":
            _ENG[which] = (O.make_plan(), NSGTBase("bark", 262, 32.9, device="cuda"))
        else:
            _ENG[which] = (mel_plan(), NSGTBase("mel", 32, 115.5, device="cuda"))
    plan, base = _ENG[which]
    return plan, base, base.nsgt


def _modules(which):
    from xumx_slicq_amd.transforms import INSGT_SL, NSGT_SL
    plan, base, eng = _setup(which)
    return plan, eng, NSGT_SL(base), INSGT_SL(base)


def _arena(eng, blocks):
    """The packed arena of a CPU block list, on the device (a copy)."""
    return torch.cat([b.float().reshape(-1) for b in blocks]).cuda()


def _judge_rows(stage, case, got, cpu, ref):
    eg, ec = ref64.rel_err(got, ref, keep=(0,)), ref64.rel_err(cpu, ref, keep=(0,))
    bad, worst = _T.judge(stage, case, eg, ec, [f"row {r}" for r in range(ref.shape[0])])
    assert not bad, "\n".join(bad[:20])
    return worst


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------
def _judge_forward_adjoint(which, BC, n, stage, case, shape_cotangent=None):
    plan, _, eng = _setup(which)
    S = plan.nslices(n)
    G = random_cotangents(plan, BC, S, seed=BC * 1000 + n % 997)
    if shape_cotangent is not None:
        shape_cotangent(plan, G)
    ref = autograd_forward_adjoint(plan, G, n)
    G32 = [g.float() for g in G]
    cpu = forward_adjoint_closed_form(plan, G32, n, dtype=F32)
    got = eng.forward_adjoint(_arena(eng, G32), (BC,), n)
    assert got.shape == (BC, n) and got.dtype == F32 and bool(torch.isfinite(got).all())
    return _judge_rows(stage, case, got.cpu(), cpu, ref)


@pytest.mark.parametrize("BC,n,S", [(8, 9031, 3), (8, 44100, 6), (3, 70000, 9)])
def test_forward_adjoint_is_at_fp32_rounding_of_float64_autograd(BC, n, S):
    """Bark-262 (hand-written slice FFT, radix-4 and dense band kernels): the smallest and odd length (n % 4 == 3), both slice
    parities, and a row count that is no multiple of anything."""
    assert _setup("bark")[0].nslices(n) == S
    _judge_forward_adjoint("bark", BC, n, "fwd_adjoint", f"bark BC {BC} n {n}")


def test_forward_adjoint_on_the_rocfft_path():
    _judge_forward_adjoint("mel", 8, 32768, "fwd_adjoint/rocfft", "mel BC 8 n 32768")


def _edge_bands_only(plan, G):
    """Non-zero only in the DC, first, last and Nyquist bands: every term of the answer passes through the fold's bands."""
    keep = {0, 1, plan.nbands - 2, plan.nbands - 1}
    for (j0, F, T), g in zip(plan.blocks, G):
        for f in range(F):
            if j0 + f not in keep:
                g[:, f] = 0


@pytest.mark.parametrize("which,BC,n", [("bark", 8, 9031), ("mel", 8, 32768)])
def test_forward_adjoint_of_the_edge_bands_alone(which, BC, n):
    _judge_forward_adjoint(which, BC, n, "fwd_adjoint" if which == "bark" else "fwd_adjoint/rocfft", f"{which} BC {BC} n {n} edge bands only",
                           _edge_bands_only)


def test_forward_adjoint_of_one_single_band_block():
    def one_block(plan, G):
        b = max((T, i) for i, (_, F, T) in enumerate(plan.blocks) if F == 1)[1]
        for i, g in enumerate(G):
            if i != b:
                g.zero_()
    _judge_forward_adjoint("bark", 8, 9031, "fwd_adjoint", "bark BC 8 n 9031 one F = 1 block", one_block)


# ---- 2. through autograd --------------------------------------------------------------------------------------------
def test_nsgt_backward_packs_a_subset_of_blocks_and_equals_the_kernel():
    plan, eng, nsgt, _ = _modules("bark")
    B, n = 2, 9031
    S = plan.nslices(n)
    touched = (0, 5, 33, len(plan.blocks) - 1)
    G = random_cotangents(plan, 2 * B, S, seed=11)
    for i, g in enumerate(G):
        if i not in touched:
            g.zero_()
    x = torch.randn(B, 2, n, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_(True)
    seen = []
    pack = eng.table.pack_grads
    eng.table.pack_grads = lambda grads, *a: (seen.append([g is None for g in grads]), pack(grads, *a))[1]
    try:
        blocks = nsgt(x)
        assert all(b.grad_fn is not None for b in blocks) and len({b.grad_fn for b in blocks}) == 1       # one node
        sum((blocks[i] * G[i].float().reshape(blocks[i].shape).cuda()).sum() for i in touched).backward()
    finally:
        del eng.table.pack_grads
    assert seen == [[i not in touched for i in range(len(plan.blocks))]]            # the others arrived as None
    want = eng.forward_adjoint(_arena(eng, G), (B, 2), n)
    assert x.grad.dtype == F32 and torch.equal(x.grad, want)
    ref = autograd_forward_adjoint(plan, G, n)
    cpu = forward_adjoint_closed_form(plan, [g.float() for g in G], n, dtype=F32)
    _judge_rows("fwd_adjoint", "bark B 2 n 9031 through NSGT_SL, four blocks", x.grad.reshape(2 * B, n).cpu(), cpu, ref)


def test_nsgt_gradient_comes_back_in_the_dtype_of_the_input():
    _, eng, nsgt, _ = _modules("bark")
    x = torch.randn(1, 2, 9031, generator=torch.Generator().manual_seed(2), dtype=F64).cuda().requires_grad_(True)
    blocks = nsgt(x)
    assert blocks[0].dtype == F32                   # cast as without grad
    blocks[3].sum().backward()
    x32 = x.detach().float().requires_grad_(True)
    nsgt(x32)[3].sum().backward()
    assert x.grad.dtype == F64 and torch.equal(x.grad, x32.grad.double())


@pytest.mark.parametrize("lead", [(2, 2), (4, 1, 2)])
@pytest.mark.parametrize("as_views", [True, False])
def test_insgt_backward_equals_backward_adjoint(lead, as_views):
    plan, eng, _, insgt = _modules("bark")
    n = 9031
    S = plan.nslices(n)
    BC = int(np.prod(lead))
    arena = torch.randn(eng.table.numel(BC, S), generator=torch.Generator().manual_seed(5)).cuda()
    views = eng.table.views(arena, lead, S)
    Y = [(v.detach() if as_views else v.clone()).requires_grad_(True) for v in views]
    w = torch.randn(*lead, n, generator=torch.Generator().manual_seed(6)).cuda()
    y = insgt(Y, n)
    assert y.shape == (*lead, n) and y.grad_fn is not None
    assert torch.equal(y.detach(), eng.backward(arena, BC, S, n).view(*lead, n))
    (y * w).sum().backward()
    want = eng.table.views(eng.backward_adjoint(w.reshape(BC, n), S), lead, S)
    for b, (Yb, gb) in enumerate(zip(Y, want)):
        assert Yb.grad.shape == Yb.shape and torch.equal(Yb.grad, gb), b


def test_gradient_of_the_round_trip_is_the_identity():
    """<w, insgt(nsgt(x), n)> has gradient w: perfect reconstruction makes the chain the identity, so its adjoint is the
    identity too -- to the round-trip error of the forward pair on the same signal, measured here; twice it is allowed.
    Measured on MI355X: round trip 2.29e-7 RMS / 1.14e-6 max relative, gradient of the chain 2.33e-7 / 1.33e-6."""
    _, eng, nsgt, insgt = _modules("bark")
    from xumx_slicq_amd.synth import synth_audio
    n = 44100
    w = synth_audio(n, seed=77, nb_samples=2).cuda()
    with torch.no_grad():
        rt = ref64.rel_err(insgt(nsgt(w), n), w)
    x = w.clone().requires_grad_(True)
    blocks = nsgt(x)
    arena, _, _ = eng.table.as_arena(blocks)
    assert arena.data_ptr() == blocks[0].data_ptr()             # the inverse reuses the arena of the forward node
    (insgt(blocks, n) * w).sum().backward()
    e = ref64.rel_err(x.grad, w)
    print(f"round trip: rel rms {float(rt[0]):.3e} max {float(rt[1]):.3e}; gradient of the chain: rel rms {float(e[0]):.3e} max {float(e[1]):.3e}")
    assert float(e[0]) <= 2 * float(rt[0]) and float(e[1]) <= 2 * float(rt[1])


def _magnitude_loss(blocks_a, blocks_b):
    return sum(((torch.abs(torch.view_as_complex(a)) - torch.abs(torch.view_as_complex(b))) ** 2).mean() for a, b in zip(blocks_a, blocks_b))


def test_gradient_of_the_magnitude_loss_against_float64_autograd_through_the_oracle():
    plan, eng, nsgt, _ = _modules("bark")
    from xumx_slicq_amd.synth import synth_audio
    from xumx_slicq_amd.transforms import ComplexNorm
    B, n = 2, 9031
    y = synth_audio(n, seed=31, nb_samples=B)
    yh = (0.8 * y + 0.1 * synth_audio(n, seed=32, nb_samples=B)).contiguous()
    grads = {}
    for dt, fwd in ((F64, ref64.forward), (F32, O.forward)):
        v = yh.to(dt).clone().requires_grad_(True)
        _magnitude_loss(fwd(plan, v), [b.detach() for b in fwd(plan, y.to(dt))]).backward()
        grads[dt] = v.grad.reshape(2 * B, n)
    v = yh.cuda().requires_grad_(True)
    norm = ComplexNorm()
    with torch.no_grad():
        target = norm(nsgt(y.cuda()))
    sum(((a - b) ** 2).mean() for a, b in zip(norm(nsgt(v)), target)).backward()
    _judge_rows("magnitude_loss", "bark B 2 n 9031", v.grad.reshape(2 * B, n).cpu(), grads[F32], grads[F64])


# ---- 3. no change without grad --------------------------------------------------------------------------------------
def test_grad_off_paths_are_bitwise_the_direct_calls():
    plan, eng, nsgt, insgt = _modules("bark")
    n = 9031
    x = torch.randn(2, 2, n, generator=torch.Generator().manual_seed(8)).cuda()
    arena, lead, S = eng.forward(x)
    want_y = eng.backward(arena, 4, S, n).view(2, 2, n)
    xg = x.clone().requires_grad_(True)
    for inp, ctx in ((x, torch.enable_grad()), (x, torch.no_grad()), (xg, torch.no_grad())):
        with ctx:
            blocks = nsgt(inp)
            y = insgt(blocks, n)
        assert all(b.grad_fn is None and not b.requires_grad for b in blocks) and y.grad_fn is None
        for b, v in zip(blocks, eng.table.views(arena, lead, S)):
            assert torch.equal(b, v)
        assert torch.equal(y, want_y)
        got, _, _ = eng.table.as_arena(blocks)
        assert got.data_ptr() == blocks[0].data_ptr()           # as_arena stays zero-copy for a run of views
    # the differentiable path computes the same bits
    blocks = nsgt(xg)
    y = insgt(blocks, n)
    assert torch.equal(torch.cat([b.detach().reshape(-1) for b in blocks]), arena) and torch.equal(y.detach(), want_y)
    # blocks that require no grad under grad mode: no node either
    y2 = insgt([b.detach() for b in blocks], n)
    assert y2.grad_fn is None and torch.equal(y2, want_y)


def _chain_gradient(nsgt, insgt, x0, w):
    x = x0.clone().requires_grad_(True)
    blocks = nsgt(x)
    (insgt([b * 0.5 for b in blocks], x0.shape[-1]) * w).sum().backward()       # (scaled blocks: the packing under grad runs too)
    return x.grad


def test_two_backward_passes_are_bitwise_equal_and_streams_agree():
    _, eng, nsgt, insgt = _modules("bark")
    g = torch.Generator().manual_seed(9)
    x0, w = torch.randn(2, 2, 9031, generator=g).cuda(), torch.randn(2, 2, 9031, generator=g).cuda()
    a = _chain_gradient(nsgt, insgt, x0, w)
    b = _chain_gradient(nsgt, insgt, x0, w)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _chain_gradient(nsgt, insgt, x0, w)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, c)


def test_double_backward_raises_naming_the_transform():
    plan, eng, nsgt, insgt = _modules("bark")
    x = torch.randn(1, 2, 9031, generator=torch.Generator().manual_seed(10)).cuda().requires_grad_(True)
    loss = sum((b ** 2).sum() for b in nsgt(x))
    with pytest.raises(RuntimeError, match="NSGT_SL"):
        torch.autograd.grad(loss, x, create_graph=True)
    S = plan.nslices(9031)
    Y = [torch.randn(1, 2, F, S, T, 2, device="cuda", requires_grad=True) for (_, F, T) in plan.blocks]
    with pytest.raises(RuntimeError, match="INSGT_SL"):
        torch.autograd.grad((insgt(Y, 9031) ** 2).sum(), Y[0], create_graph=True)
