"""Time Separator.remix against forward on the bench shape: one seeded 240 s stereo track (10,584,000 samples), the offline
model, mix-phase (BASELINE configs[1]) and Wiener-EM (configs[2]), chunk_size 2,621,440.

Arms, each warmed up and timed with HIP events on the caller's stream, alternated round by round (so drift lands on
every arm alike):
    forward           the four stems
    forward+einsum    the stems, then the R = 2 vocals / accompaniment mix as a torch einsum (what a caller did before)
    remix_R1          karaoke: {"vocals": 0}
    remix_R2          vocals / accompaniment: [[0, 1, 0, 0], [1, 0, 1, 1]]
    remix_R4          identity gains (the four stems through remix)
One JSON line per (mode, arm): median / min / max milliseconds over the rounds, and the per-kernel times of one more call
of the arm from the library's event profiler (xsq_profile_*).  --samples DIR writes a seeded sample of every arm's output
(DIR/remix_samples_<mode>.npz), so the arms can be compared with each other.

    python tools/remix_bench.py [--rounds 7] [--iters 5] [--modes phasemix wiener] [--samples DIR]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

TRACK_SAMPLES = 10_584_000
CHUNK = 2_621_440
AGG = [[0, 1, 0, 0], [1, 0, 1, 1]]


def arms(sep):
    G2 = torch.tensor(AGG, dtype=torch.float32)
    return {
        "forward": lambda x: sep(x),
        "forward+einsum": lambda x: torch.einsum("rt,tbcn->rbcn", G2.to(x.device), sep(x)),
        "remix_R1": lambda x: sep.remix(x, {"vocals": 0}),
        "remix_R2": lambda x: sep.remix(x, AGG),
        "remix_R4": lambda x: sep.remix(x, torch.eye(4)),
    }


def time_once(fn, x, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["phasemix", "wiener"], choices=["phasemix", "wiener"])
    ap.add_argument("--arms", nargs="+", default=None, help="a subset of the arms (default: all)")
    ap.add_argument("--samples", type=str, default=None, help="directory for a seeded sample of every arm's output")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel profile call")
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.synth import synth_audio
    dev = torch.device("cuda", 0)
    x = synth_audio(TRACK_SAMPLES, seed=20260101).to(dev)
    pick = np.sort(np.random.default_rng(20260101).choice(TRACK_SAMPLES, 4096, replace=False))
    for mode in args.modes:
        sep = seeded_separator(realtime=False, wiener=(mode == "wiener"), device=dev, chunk_size=CHUNK)
        table = arms(sep)
        names = [a for a in table if args.arms is None or a in args.arms]
        samples = {}
        for name in names:                          # warm-up: caches, workspaces, plans of every arm
            for _ in range(args.warmup):
                out = table[name](x)
            torch.cuda.synchronize()
            samples[name] = out[..., torch.from_numpy(pick).to(dev)].cpu().numpy()
            del out
        times = {name: [] for name in names}
        for _ in range(args.rounds):
            for name in names:
                times[name].append(time_once(table[name], x, args.iters))
        kern = {}
        if not args.no_kernels:
            for name in names:
                _lib.profile_reset()
                _lib.profile_enable(True)
                table[name](x)
                torch.cuda.synchronize()
                kern[name] = {k: round(v[0], 4) for k, v in sorted(_lib.profile_read().items())}
                _lib.profile_enable(False)
        for name in names:
            t = np.array(times[name])
            print(json.dumps({"tool": "remix_bench", "mode": mode, "arm": name, "samples": TRACK_SAMPLES, "chunk_size": CHUNK,
                              "rounds": args.rounds, "iters": args.iters, "ms_median": round(float(np.median(t)), 4),
                              "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                              "vs_forward": round(float(np.median(t)) / float(np.median(times["forward"])), 4)
                              if "forward" in times else None,
                              "kernels_ms": kern.get(name)}), flush=True)
        if args.samples:
            os.makedirs(args.samples, exist_ok=True)
            np.savez(os.path.join(args.samples, f"remix_samples_{mode}.npz"), index=pick,
                     **{k.replace("+", "_"): v for k, v in samples.items()})
        del sep, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
