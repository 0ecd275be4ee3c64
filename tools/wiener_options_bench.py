"""Time Separator.forward under the Wiener filter's option sets on the bench shape: one seeded 240 s stereo track (10,584,000
samples), the offline model, chunk_size 2,621,440.

Arms: niter in {1, 2} x (softmask, residual) in {00, 10, 01, 11}, the native call, each warmed up and timed with HIP events on the
caller's stream, alternated round by round in ONE process (so drift lands on every arm alike).  The rows with both flags off are the
arms ``niter1`` and ``niter2_native`` of tools/wiener_iters_bench.py (profiles/wiener_iters_bench.jsonl).  One JSON line per arm,
appended to --out (default profiles/wiener_options_bench.jsonl): median / min / max milliseconds over the rounds, the per-kernel
times of one more call from the library's event profiler (the Wiener kernels and the inverse transform's), the form the EM took
and the HBM bytes per time-frequency point of that form (from the code: masks 32 B, mix 16 B, estimates 16 B per source).

    python tools/wiener_options_bench.py [--rounds 7] [--iters 5] [--out FILE]
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


def em_form(niter, J):
    """The form ``auto`` takes at the default window of 5000 frames."""
    from xumx_slicq_amd.phase import resident_max_window
    if niter <= 1:
        return "three launches" if niter else "start"
    return "resident" if resident_max_window(J) >= 5000 else "looped"


def em_bytes_per_point(niter, J, form):
    """One iteration from masks: statistics (16 + 32) + apply (16 + 32 read, 16 J written); a further looped iteration: statistics
    of Y (16 J) + apply (16 + 16 J read, 16 J written); resident: window maximum (16) + one read (16 + 32) + one write (16 J)."""
    if niter == 0:
        return 48 + 16 * J
    if form == "resident":
        return 64 + 16 * J
    return 96 + 16 * J + (niter - 1) * (16 + 48 * J)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "wiener_options_bench.jsonl"))
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.synth import synth_audio
    dev = torch.device("cuda", 0)
    x = synth_audio(TRACK_SAMPLES, seed=20260101).to(dev)
    sep = seeded_separator(realtime=False, device=dev, chunk_size=CHUNK)
    table = [(f"niter{k}_s{s}r{r}", k, s, r) for k in (1, 2) for s, r in ((0, 0), (1, 0), (0, 1), (1, 1))]

    def call(arm):
        _, k, s, r = arm
        sep.niter, sep.softmask, sep.residual = k, bool(s), bool(r)
        return sep(x)

    def time_once(arm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call(arm)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    for arm in table:                              # warm-up: caches, workspaces, plans of every arm
        for _ in range(args.warmup):
            call(arm)
        torch.cuda.synchronize()
    times = {arm[0]: [] for arm in table}
    for _ in range(args.rounds):
        for arm in table:
            times[arm[0]].append(time_once(arm))
    kern = {}
    for arm in table:
        _lib.profile_reset()
        _lib.profile_enable(True)
        call(arm)
        torch.cuda.synchronize()
        kern[arm[0]] = {k: round(v[0], 4) for k, v in sorted(_lib.profile_read().items())}
        _lib.profile_enable(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, k, s, r in table:
            t = np.array(times[name])
            J = 5 if r else 4
            form = em_form(k, J)
            wk = {n: v for n, v in kern[name].items() if n.startswith("wiener")}
            line = json.dumps({"tool": "wiener_options_bench", "arm": name, "niter": k, "softmask": s, "residual": r, "form": form,
                               "samples": TRACK_SAMPLES, "chunk_size": CHUNK, "rounds": args.rounds, "iters": args.iters,
                               "ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4),
                               "ms_max": round(float(t.max()), 4), "em_bytes_per_point": em_bytes_per_point(k, J, form),
                               "wiener_kernels_ms": wk, "wiener_kernels_ms_sum": round(sum(wk.values()), 4),
                               "other_kernels_ms": {n: v for n, v in kern[name].items() if not n.startswith("wiener")}})
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
