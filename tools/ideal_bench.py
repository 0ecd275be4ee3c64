"""Time the ideal-mask oracle as one native call against the same oracle composed from the modules that existed before it, on
Bark-262 and two shapes: one full chunk (B = 1, 2,621,440 stereo samples, S = 292) and sixteen two-second rows (B = 16,
88,200 samples, S = 11).

Arms, each warmed up, alternated round by round (so drift lands on every arm alike) and timed with HIP events; the median over
the rounds is reported:
    ideal/<strategy>      slicqfinder.ideal_slicqt: xsq_ideal_separate (forward of the 8B rows, filter in place, inverse)
    composed/<strategy>   NSGT_SL on the four stems -> ComplexNorm -> sum over the stems + 5e-10 -> phase.wiener /
                          phase.phasemix_sep -> INSGT_SL: the parent's code, block by block
    filter/<strategy>     the filter alone on an arena that is already there (slicqfinder.filter_sources_arena, out of place), with
                          its kernels' own times from the library's event profiler (wiener_stats, wiener_finalize, wiener_apply,
                          phasemix_sources).  Its rate is the bytes the algorithm must move -- per point and stereo channel the
                          four sources' coefficients in and the four estimates out, 64 B, and for ``wiener`` the coefficients
                          once more for the statistics, 96 B -- over that time, printed beside the 6.29 TB/s a float4 copy
                          reaches on this part.  ``working_set_mb`` against the 256 MiB Infinity Cache says where it reads from.
    search-step           one TrackEvaluator.oracle round (Bark-262, two seeded 30 s tracks) in tracks per second, host clock
                          around work that ends in a device-to-host read; the plan build and the table upload are timed apart.
Before anything is timed the two routes are compared on the same input (``max_abs_diff``).

One JSON line per (shape, arm), appended to --out as well.

    python tools/ideal_bench.py [--rounds 7] [--iters 3] [--out profiles/ideal_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {"chunk": (1, 2_621_440), "rows16x2s": (16, 88_200)}
PLAN = ("bark", 262, 32.9)
BYTES_PER_POINT_CHANNEL = {"wiener": 96, "phasemix": 64}
HBM_COPY_TBS, HBM_SPEC_TBS, INFINITY_CACHE_MB = 6.29, 8.0, 256 * 1.048576
EPS = 1.0e-10


def event_timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-search-step", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "ideal_bench.jsonl"))
    args = ap.parse_args()

    from xumx_slicq_amd import _lib, phase
    from xumx_slicq_amd.data import DeviceDataset
    from xumx_slicq_amd.slicqfinder import TrackEvaluator, filter_sources_arena, ideal_slicqt
    from xumx_slicq_amd.synth import synth_audio, synth_audio_device
    from xumx_slicq_amd.transforms import ComplexNorm, NSGTBase, make_filterbanks
    dev = torch.device("cuda", 0)
    base = NSGTBase(*PLAN, device=dev)
    eng = base.nsgt
    nsgt, insgt = make_filterbanks(base)
    cnorm = ComplexNorm()

    def composed(src, strategy):
        C = nsgt(src)
        mags = cnorm(C)
        mix = [blk.sum(0) + 5 * EPS for blk in C]
        Y = phase.wiener(mix, mags) if strategy == "wiener" else phase.phasemix_sep(mix, mags)
        return insgt(Y, src.shape[-1])

    lines = []
    for shape in args.shapes:
        B, n = SHAPES[shape]
        src = torch.stack([g * synth_audio_device(n, 20260300 + j, dev, nb_samples=B) for j, g in enumerate((0.5, 0.35, 0.25, 0.4))])
        arena, _, S = eng.forward(src)
        arena2 = torch.empty_like(arena)
        points = B * 2 * S * eng.table.coefs_per_slice
        arms, diff = {}, {}
        for strategy in ("wiener", "phasemix"):
            arms[f"ideal/{strategy}"] = lambda s=strategy: ideal_slicqt(src, base, s)
            arms[f"composed/{strategy}"] = lambda s=strategy: composed(src, s)
            arms[f"filter/{strategy}"] = lambda s=strategy: filter_sources_arena(eng.table, arena, arena2, B, S, s)
            diff[strategy] = float((ideal_slicqt(src, base, strategy) - composed(src, strategy)).abs().max())
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                times[name].append(event_timed(fn, args.iters))
        kern = {}
        for strategy in ("wiener", "phasemix"):
            _lib.profile_reset()
            _lib.profile_enable(True)
            for _ in range(args.rounds):
                arms[f"filter/{strategy}"]()
            torch.cuda.synchronize()
            kern[strategy] = {k: v[0] / max(v[1], 1) for k, v in _lib.profile_read().items() if k.startswith(("wiener_", "phasemix_"))}
            _lib.profile_enable(False)
        med = {name: float(np.median(t)) for name, t in times.items()}
        for name, t in times.items():
            t = np.array(t)
            kind, strategy = name.split("/")
            line = {"tool": "ideal_bench", "plan": list(PLAN), "shape": shape, "B": B, "samples": n, "slices": S, "arm": name,
                    "rounds": args.rounds, "clock": "hip-events", "ms_median": round(med[name], 4), "ms_min": round(float(t.min()), 4),
                    "ms_max": round(float(t.max()), 4), "max_abs_diff_ideal_vs_composed": diff[strategy]}
            if kind == "ideal":
                line["composed_over_ideal"] = round(med[f"composed/{strategy}"] / med[name], 3)
            if kind == "filter":
                nbytes = points * BYTES_PER_POINT_CHANNEL[strategy]
                ms = sum(kern[strategy].values())
                line.update({"kernels_ms": {k: round(v, 5) for k, v in sorted(kern[strategy].items())}, "bytes": nbytes,
                             "working_set_mb": round(points * 64 / 1e6, 1), "fits_infinity_cache": points * 64 / 1e6 < INFINITY_CACHE_MB,
                             "kernels_tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3) if ms else None,
                             "hbm_copy_tb_per_s": HBM_COPY_TBS, "hbm_spec_tb_per_s": HBM_SPEC_TBS})
            lines.append(line)
            print(json.dumps(line), flush=True)
        del src, arena, arena2, arms
        torch.cuda.empty_cache()

    if not args.no_search_step:
        n = 30 * 44100
        tracks = [{s: (g * synth_audio(n, seed=20260400 + 10 * t + j)[0]).numpy()
                   for j, (s, g) in enumerate(zip(DeviceDataset.sources, (0.5, 0.35, 0.25, 0.4)))} for t in range(2)]
        ds = DeviceDataset.from_arrays(tracks, storage="fp32", device=dev)
        ev = TrackEvaluator(ds)
        ev.oracle(*PLAN[:1], PLAN[2], PLAN[1])                      # warm-up: code objects, rocFFT plans of other shapes
        build, upload, step = [], [], []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b2 = NSGTBase(*PLAN, device=dev)
            t1 = time.perf_counter()
            b2.nsgt.demixer(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            del b2
            sdr = ev.oracle(*PLAN[:1], PLAN[2], PLAN[1])            # (builds and frees its own plan: included)
            t3 = time.perf_counter()
            build.append((t1 - t0) * 1e3); upload.append((t2 - t1) * 1e3); step.append((t3 - t2) * 1e3)
        line = {"tool": "ideal_bench", "plan": list(PLAN), "shape": "search-step", "tracks": len(ds), "samples": n, "arm": "TrackEvaluator.oracle",
                "rounds": args.rounds, "clock": "host+device-to-host read", "ms_median": round(float(np.median(step)), 3),
                "tracks_per_s": round(len(ds) / (float(np.median(step)) * 1e-3), 3), "plan_build_ms_median": round(float(np.median(build)), 3),
                "plan_upload_ms_median": round(float(np.median(upload)), 3), "sdr": list(sdr)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
