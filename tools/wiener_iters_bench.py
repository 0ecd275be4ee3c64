"""Time Separator.forward at several Wiener-EM iteration counts on the bench shape: one seeded 240 s stereo track (10,584,000
samples), the offline model, chunk_size 2,621,440.

Arms, each warmed up and timed with HIP events on the caller's stream, alternated round by round in ONE process (so drift
lands on every arm alike):
    niter0 / niter1             the native call at 0 (mix-phase) and 1 iteration: the yardsticks, the kernels of bench.py and
                                bench.py --wiener
    niter1_module               one iteration through the module-API schedule (``native = False``): the yardstick of the two
                                arms below, which take that schedule because a method other than "auto" is an A/B switch
    niterK_resident_module      K in {2, 3, 5}: the window-resident kernel
    niterK_looped_module        K in {2, 3, 5}: iteration 1 as ever, then statistics + apply per iteration
    niterK_native               K in {2, 3, 5}: the native call (method auto = resident at the default window)
One JSON line per arm, appended to --out (default profiles/wiener_iters_bench.jsonl): median / min / max milliseconds over the
rounds, the per-kernel times of one more call from the library's event profiler, and the HBM bytes per time-frequency point
of the arm's EM form (from the code: masks 32 B, mix 16 B, estimates 64 B per point).

    python tools/wiener_iters_bench.py [--rounds 7] [--iters 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

TRACK_SAMPLES = 10_584_000
CHUNK = 2_621_440
KS = (2, 3, 5)


def em_bytes_per_point(niter, method):
    """HBM bytes per time-frequency point of the masked EM: one iteration = statistics (16 + 32) + apply (16 + 32 read, 64
    written) = 160; a further looped iteration = statistics of Y (64) + apply (16 + 64 read, 64 written) = 208; resident =
    window maximum (16) + one read (16 + 32) + one write (64) = 128 whatever niter is."""
    if niter == 0:
        return 0
    if niter == 1:
        return 160
    return 128 if method == "resident" else 160 + 208 * (niter - 1)


def arms():
    out = [("niter0", 0, "auto", True), ("niter1", 1, "auto", True), ("niter1_module", 1, "auto", False)]
    for k in KS:
        out += [(f"niter{k}_resident_module", k, "resident", False), (f"niter{k}_looped_module", k, "looped", False),
                (f"niter{k}_native", k, "auto", True)]
    return out


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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "wiener_iters_bench.jsonl"))
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.synth import synth_audio
    dev = torch.device("cuda", 0)
    x = synth_audio(TRACK_SAMPLES, seed=20260101).to(dev)
    sep = seeded_separator(realtime=False, device=dev, chunk_size=CHUNK)
    table = arms()

    def call(arm):
        _, k, method, native = arm

        def fn(a):
            sep.niter, sep.xumx_model.niter_method, sep.native = k, method, native
            return sep(a)
        return fn

    for arm in table:                              # warm-up: caches, workspaces, plans of every arm
        for _ in range(args.warmup):
            call(arm)(x)
        torch.cuda.synchronize()
    times = {arm[0]: [] for arm in table}
    for _ in range(args.rounds):
        for arm in table:
            times[arm[0]].append(time_once(call(arm), x, args.iters))
    kern = {}
    for arm in table:
        _lib.profile_reset()
        _lib.profile_enable(True)
        call(arm)(x)
        torch.cuda.synchronize()
        kern[arm[0]] = {k: round(v[0], 4) for k, v in sorted(_lib.profile_read().items()) if k.startswith("wiener")}
        _lib.profile_enable(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, k, method, native in table:
            t = np.array(times[name])
            form = ("resident" if method != "looped" else "looped") if k >= 2 else ("three launches" if k == 1 else "none")
            line = json.dumps({"tool": "wiener_iters_bench", "arm": name, "niter": k, "form": form,
                               "schedule": "native" if native else "module", "samples": TRACK_SAMPLES, "chunk_size": CHUNK,
                               "rounds": args.rounds, "iters": args.iters, "ms_median": round(float(np.median(t)), 4),
                               "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                               "em_bytes_per_point": em_bytes_per_point(k, form), "wiener_kernels_ms": kern[name],
                               "wiener_kernels_ms_sum": round(sum(kern[name].values()), 4)})
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
