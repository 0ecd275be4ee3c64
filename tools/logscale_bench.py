"""Time the transforms and the ideal-mask oracle on two plans with long bands -- C = ``cqlog, 12, 20.0`` (Lg up to 6416) and
``cqlog, 48, 32.9`` (21 long bands up to 5004) -- against the same transform composed from torch ops on the device, on two shapes: one
full chunk (B = 1, 2,621,440 stereo samples) and sixteen two-second rows (B = 16, 88,200 samples).

Arms, each warmed up, alternated round by round (so drift lands on every arm alike) and timed with HIP events; the median over the
rounds is reported with the smallest and the largest round:
    forward/native    NSGT_SL (xsq_slicqt_forward)               forward/torch   slices * slice window -> torch.fft.fft (COMPLEX, over the
                                                                                 real slices, as the reference's nsgtf does: about twice the
                                                                                 slice-FFT work an rfft with a mirrored gather would need) ->
                                                                                 per block the gathered bins * analysis windows -> torch.fft.ifft
    inverse/native    INSGT_SL (xsq_slicqt_inverse)              inverse/torch   per block torch.fft.fft * dual windows -> index_add into the
                                                                                 slice spectra -> torch.fft.irfft -> overlap-add
    wiener/native     slicqfinder.ideal_slicqt (one call)        wiener/torch    the torch forward of the four stems -> phase.wiener (the
                                                                                 package's own NATIVE filter: the two arms differ in the
                                                                                 transforms and the glue between the calls only) -> the torch inverse
``engine_share``: the FFT band engine's kernels (band_analysis_fft / band_synthesis_fft) over all kernels of the native transform, from
the library's event profiler.  Before anything is timed the two routes are compared on the same input (``max_abs_diff``).
``--draws N``: of the first N ``cqlog`` draws of the search's default ranges (seed 42), how many ``build_plan(long_bands=True,
dc_twins=True)`` accepts at the engine's maximum with sllen <= 44100, and why the others are refused (host only).

One JSON line per (plan, shape, arm), appended to --out as well.

    python tools/logscale_bench.py [--rounds 7] [--iters 2] [--out profiles/logscale_bench.jsonl]

``--net``: instead of the above, ``Separator.forward`` of the seeded offline model (Wiener-EM) with ``long_bands=True`` on the same two
plans and shapes, two arms alternated round by round:
    separator/fused   the default: the analysis kernels (the FFT band engine among them) write the CDAE's whitened magnitude
    separator/two_pass  ``fuse_whiten = False``: the Python chunk loop, the model's own magnitude pass
each with the per-kernel table of one call from the library's event profiler (``kernels_ms``) and the device memory the model's weight
pools take (``weight_pools_bytes``: what ``xsq_model_create`` allocates, read from the driver's free-memory count).

    python tools/logscale_bench.py --net [--out profiles/logscale_net_bench.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {"chunk": (1, 2_621_440), "rows16x2s": (16, 88_200)}
PLANS = {"C": ("cqlog", 12, 20.0), "cqlog48": ("cqlog", 48, 32.9)}


def event_timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


class TorchSliCQ:
    """The transform of ``plan`` composed from torch ops on ``dev`` (the closed forms of oracle/slicqt.py, complex64)."""

    def __init__(self, plan, dev):
        self.p, self.dev = plan, dev
        L = plan.L
        off = np.concatenate(([0], np.cumsum(plan.Lg)))
        self.tw = torch.from_numpy(plan.tw).to(dev)
        self.blocks = []
        for (j0, F, T) in plan.blocks:
            q = np.arange(T)
            sq = np.where(q < (T + 1) // 2, q, q - T)
            k = plan.c[j0:j0 + F, None].astype(np.int64) + sq[None, :]
            sign = np.where((plan.c[j0:j0 + F] // 2) % 2 == 0, 1.0, -1.0)[:, None]
            g = np.stack([plan.g[off[j]: off[j + 1]] for j in range(j0, j0 + F)]) * sign
            gd = np.stack([plan.gd[off[j]: off[j + 1]] for j in range(j0, j0 + F)]) * sign * T
            keep = (k >= 0) & (k <= L // 2)
            self.blocks.append((F, T, torch.from_numpy(k % L).to(dev), torch.from_numpy(g.astype(np.float32)).to(dev),
                                torch.from_numpy(np.where(keep, gd, 0.0).astype(np.float32)).to(dev),
                                torch.from_numpy(np.where(keep, k, 0)).to(dev)))

    def forward(self, x):
        p = self.p
        lead, n = x.shape[:-1], x.shape[-1]
        xb = x.reshape(-1, n)
        S, h = p.num_slices(n), p.hop
        pad = torch.zeros(xb.shape[0], (2 * S + 2) * h, dtype=torch.float32, device=self.dev)
        pad[:, 2 * h: 2 * h + n] = xb
        U = torch.fft.fft(pad.unfold(-1, p.L, 2 * h)[:, :S] * self.tw)                   # (BC, S, L)
        out = []
        for (F, T, k, g, _gd, _kk) in self.blocks:
            cb = torch.fft.ifft(U[:, :, k] * g).permute(0, 2, 1, 3).contiguous()         # (BC, F, S, T)
            out.append(torch.view_as_real(cb).reshape(*lead, F, S, T, 2))
        return out

    def inverse(self, X, n):
        p = self.p
        lead, S = X[0].shape[:-4], X[0].shape[-3]
        BC = int(np.prod(lead)) if len(lead) else 1
        fr = torch.zeros(BC, S, p.L // 2 + 1, dtype=torch.complex64, device=self.dev)
        for (F, T, _k, _g, gd, kk), Xb in zip(self.blocks, X):
            fc = torch.fft.fft(torch.view_as_complex(Xb.reshape(BC, F, S, T, 2).contiguous())) * gd[None, :, None, :]
            fr.index_add_(2, kk.reshape(-1), fc.permute(0, 2, 1, 3).reshape(BC, S, F * T))
        seg = torch.fft.irfft(fr, n=p.L)
        h = p.hop
        y = torch.zeros(BC, (2 * S + 2) * h, dtype=torch.float32, device=self.dev)
        for par in (0, 1):                                                                # slices of one parity do not overlap
            sl = seg[:, par::2]
            y[:, 2 * par * h: 2 * par * h + sl.shape[1] * p.L] += sl.reshape(BC, -1)
        return y[:, 2 * h: 2 * h + n].reshape(*lead, n)


def draw_census(count):
    from xumx_slicq_amd.plan import build_plan, long_band_max
    from xumx_slicq_amd.slicqfinder import draw_params
    table = [d for d in draw_params(42, 8 * count + 64, ["bark", "mel", "cqlog"], (10, 300), (10.0, 130.0, 0.1)) if d[0] == "cqlog"][:count]
    res = {"accepted": 0, "sllen_above_44100": 0, "band_above_engine_max": 0, "band_above_half_slice": 0, "other_refusal": 0, "longest_accepted_band": 0}
    for scale, bins, fmin in table:
        try:
            p = build_plan(scale, bins, fmin, long_bands=True, dc_twins=True)
        except ValueError as e:
            why = "band_above_engine_max" if "xsq_plan_long_band_max" in str(e) else "band_above_half_slice" if "half the slice" in str(e) else "other_refusal"
            res[why] += 1
            continue
        if p.L > 44100:
            res["sllen_above_44100"] += 1
        else:
            res["accepted"] += 1
            res["longest_accepted_band"] = max(res["longest_accepted_band"], int(p.Lg.max()))
    return {"tool": "logscale_bench", "arm": "draw-census", "scale": "cqlog", "draws": len(table), "seed": 42, "engine_max": long_band_max(), **res}


def net_bench(args):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.synth import synth_audio_device
    dev = torch.device("cuda", 0)
    lines = []
    for pk in args.plans:
        scale, fbins, fmin = PLANS[pk]
        sep = seeded_separator(realtime=False, device=dev, fscale=scale, fbins=fbins, fmin=fmin, long_bands=True)
        plan = sep.nsgt.nsgt.plan
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(dev)[0]
        sep.xumx_model._model(dev)                       # xsq_model_create: the folded and the transformed weight pools
        torch.cuda.synchronize()
        pools = int(free0 - torch.cuda.mem_get_info(dev)[0])
        for shape in args.shapes:
            B, n = SHAPES[shape]
            x = synth_audio_device(n, 20260300, dev, nb_samples=B)

            def arm(fused):
                sep.fuse_whiten = fused
                return sep(x)

            arms = {"separator/fused": lambda: arm(True), "separator/two_pass": lambda: arm(False)}
            with torch.no_grad():
                a, b = arms["separator/fused"]().clone(), arms["separator/two_pass"]().clone()
                same = bool(torch.equal(a, b))
                del a, b
                for fn in arms.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = {name: [] for name in arms}
                for _ in range(args.rounds):
                    for name, fn in arms.items():
                        times[name].append(event_timed(fn, args.iters))
                kernels = {}
                for name, fn in arms.items():
                    _lib.profile_reset()
                    _lib.profile_enable(True)
                    fn()
                    torch.cuda.synchronize()
                    kernels[name] = {k: [round(float(v[0]), 4), int(v[1])] for k, v in sorted(_lib.profile_read().items())}
                    _lib.profile_enable(False)
            sep.fuse_whiten = True
            for name, t in times.items():
                t = np.array(t)
                line = {"tool": "logscale_bench", "mode": "net", "plan": list(PLANS[pk]), "L": plan.L, "longest_band": int(plan.Lg.max()),
                        "long_bands": int((plan.Lg > 320).sum()), "blocks": len(plan.blocks), "shape": shape, "B": B, "samples": n,
                        "slices": plan.num_slices(n), "arm": name, "rounds": args.rounds, "clock": "hip-events",
                        "ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                        "two_arms_bitwise_equal": same, "weight_pools_bytes": pools, "kernels_ms": kernels[name]}
                lines.append(line)
                print(json.dumps(line), flush=True)
            del x
            torch.cuda.empty_cache()
        sep.drop_graphs()
        del sep
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--plans", nargs="+", default=list(PLANS), choices=list(PLANS))
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "logscale_bench.jsonl"))
    ap.add_argument("--net", action="store_true", help="time Separator.forward on the two plans instead of the transforms")
    args = ap.parse_args()
    if args.net:
        lines = net_bench(args)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
        return

    from xumx_slicq_amd import _lib, phase
    from xumx_slicq_amd.slicqfinder import ideal_slicqt
    from xumx_slicq_amd.synth import synth_audio_device
    from xumx_slicq_amd.transforms import ComplexNorm, NSGTBase, make_filterbanks
    dev = torch.device("cuda", 0)
    cnorm = ComplexNorm()
    lines = []
    for pk in args.plans:
        base = NSGTBase(*PLANS[pk], device=dev, long_bands=True)
        nsgt, insgt = make_filterbanks(base)
        tq = TorchSliCQ(base.plan, dev)

        def torch_oracle(src):
            C = tq.forward(src)
            mix = [blk.sum(0) + 5e-10 for blk in C]
            return tq.inverse(phase.wiener(mix, cnorm(C)), src.shape[-1])

        for shape in args.shapes:
            B, n = SHAPES[shape]
            src = torch.stack([g * synth_audio_device(n, 20260300 + j, dev, nb_samples=B) for j, g in enumerate((0.5, 0.35, 0.25, 0.4))])
            x = src.sum(0)
            with torch.no_grad():
                C = [c.clone() for c in nsgt(x)]
                S = C[0].shape[-3]
                diff = {"forward": max(float((a - b).abs().max()) for a, b in zip(C, tq.forward(x))),
                        "inverse": float((insgt(C, n) - tq.inverse(C, n)).abs().max()),
                        "wiener": float((ideal_slicqt(src, base, "wiener") - torch_oracle(src)).abs().max())}
                arms = {"forward/native": lambda: nsgt(x), "forward/torch": lambda: tq.forward(x),
                        "inverse/native": lambda: insgt(C, n), "inverse/torch": lambda: tq.inverse(C, n),
                        "wiener/native": lambda: ideal_slicqt(src, base, "wiener"), "wiener/torch": lambda: torch_oracle(src)}
                for fn in arms.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = {name: [] for name in arms}
                for _ in range(args.rounds):
                    for name, fn in arms.items():
                        times[name].append(event_timed(fn, args.iters))
                share = {}
                for op in ("forward", "inverse"):
                    _lib.profile_reset()
                    _lib.profile_enable(True)
                    for _ in range(3):
                        arms[f"{op}/native"]()
                    torch.cuda.synchronize()
                    prof = {k: v[0] for k, v in _lib.profile_read().items()}
                    _lib.profile_enable(False)
                    eng = sum(v for k, v in prof.items() if k.endswith("_fft") and k.startswith("band_"))
                    share[op] = round(eng / max(sum(prof.values()), 1e-12), 4)
            med = {name: float(np.median(t)) for name, t in times.items()}
            for name, t in times.items():
                t = np.array(t)
                op, kind = name.split("/")
                line = {"tool": "logscale_bench", "plan": list(PLANS[pk]), "L": base.plan.L, "longest_band": int(base.plan.Lg.max()),
                        "long_bands": int((base.plan.Lg > 320).sum()), "shape": shape, "B": B, "samples": n, "slices": S, "arm": name,
                        "rounds": args.rounds, "clock": "hip-events", "ms_median": round(med[name], 4), "ms_min": round(float(t.min()), 4),
                        "ms_max": round(float(t.max()), 4), "max_abs_diff_native_vs_torch": diff[op]}
                if kind == "native":
                    other = np.array(times[f"{op}/torch"])
                    line["torch_over_native"] = round(med[f"{op}/torch"] / med[name], 3)
                    line["faster_by_more_than_the_spread"] = bool(t.max() < other.min())
                    if op in share:
                        line["engine_share"] = share[op]
                lines.append(line)
                print(json.dumps(line), flush=True)
            del src, x, C, arms
            torch.cuda.empty_cache()
        base.nsgt.close()
    if args.draws > 0:
        lines.append(draw_census(args.draws))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
