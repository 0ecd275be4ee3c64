"""Time the two sliCQT adjoints beside their structural twins, and a whole ``loss.backward()`` through ``insgt(nsgt(x))``.

Cases: Bark-262 at a 2-second training batch (B 16, stereo) and at one full chunk (n = 2,621,440, stereo); Mel-32 (rocFFT path) at
32,768 samples (B 16, stereo).  Arms, each warmed up and timed with HIP events on the caller's stream, alternated round by round
(so drift lands on every arm alike), medians over the rounds:
    forward_adjoint     dLoss/dcoef -> dLoss/dx   (xsq_slicqt_forward_adjoint)      twin: inverse   (xsq_slicqt_inverse_rows)
    backward_adjoint    dLoss/dy -> dLoss/dcoef   (xsq_slicqt_inverse_adjoint)      twin: forward   (xsq_slicqt_forward)
    chain_forward       insgt(nsgt(x)) with grad mode off
    chain_fwd_bwd       x.requires_grad_(); (insgt(nsgt(x)) * w).sum().backward()
One JSON line per case, appended to profiles/autograd_bench.jsonl (or --out), with the per-kernel times of one more call of each
adjoint and twin from the library's event profiler (xsq_profile_*).

    python tools/autograd_bench.py [--rounds 9] [--iters 10] [--cases bark_2s_b16 bark_chunk mel32] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = {
    "bark_2s_b16": (("bark", 262, 32.9), (16, 2), 88_200),
    "bark_chunk": (("bark", 262, 32.9), (1, 2), 2_621_440),
    "mel32": (("mel", 32, 115.5), (16, 2), 32_768),
}


def time_once(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "autograd_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("autograd_bench: needs a ROCm device (a time taken anywhere else says nothing)")

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.transforms import INSGT_SL, NSGT_SL, NSGTBase
    dev = torch.device("cuda", 0)
    for case in args.cases:
        scale, lead, n = CASES[case]
        base = NSGTBase(*scale, device="cuda")
        eng, nsgt, insgt = base.nsgt, NSGT_SL(base), INSGT_SL(base)
        BC, S = int(np.prod(lead)), base.plan.num_slices(n)
        g = torch.Generator().manual_seed(20260101)
        x = torch.randn(*lead, n, generator=g).to(dev)
        w = torch.randn(*lead, n, generator=g).to(dev)
        arena, _, _ = eng.forward(x)
        garena = torch.randn(arena.numel(), generator=g).to(dev)

        def chain_fwd_bwd():
            xg = x.detach().requires_grad_(True)
            (insgt(nsgt(xg), n) * w).sum().backward()
            return xg.grad

        def chain_forward():
            with torch.no_grad():
                return insgt(nsgt(x), n)

        arms = {
            "forward_adjoint": lambda: eng.forward_adjoint(garena, lead, n),
            "inverse": lambda: eng.backward(garena, BC, S, n),
            "backward_adjoint": lambda: eng.backward_adjoint(w.view(BC, n), S),
            "forward": lambda: eng.forward(x),
            "chain_forward": chain_forward,
            "chain_fwd_bwd": chain_fwd_bwd,
        }
        for fn in arms.values():                    # warm-up: tables built on first use, workspaces, rocFFT plans
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                times[name].append(time_once(fn, args.iters))
        kern = {}
        for name in ("forward_adjoint", "inverse", "backward_adjoint", "forward"):
            _lib.profile_reset()
            _lib.profile_enable(True)
            arms[name]()
            torch.cuda.synchronize()
            kern[name] = {k: round(v[0], 4) for k, v in sorted(_lib.profile_read().items())}
            _lib.profile_enable(False)
        med = {name: float(np.median(t)) for name, t in times.items()}
        line = {"tool": "autograd_bench", "case": case, "scale": list(scale), "lead": list(lead), "n": n, "BC": BC, "S": S,
                "fft": "lds" if base.plan.L == 18060 else "rocfft", "rounds": args.rounds, "iters": args.iters,
                "ms_median": {k: round(v, 4) for k, v in med.items()},
                "ms_min": {k: round(float(np.min(t)), 4) for k, t in times.items()},
                "ms_max": {k: round(float(np.max(t)), 4) for k, t in times.items()},
                "forward_adjoint_vs_inverse": round(med["forward_adjoint"] / med["inverse"], 4),
                "backward_adjoint_vs_forward": round(med["backward_adjoint"] / med["forward"], 4),
                "chain_fwd_bwd_vs_forward": round(med["chain_fwd_bwd"] / med["chain_forward"], 4),
                "kernels_ms": kern, "xsq_env": _lib.xsq_environment()}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del eng, nsgt, insgt, base, arena, garena, x, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
