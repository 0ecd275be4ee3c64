"""Time scoring a separation on the device against what it replaces, on two shapes: the bench track (one seeded 240 s stereo
track, 10,584,000 samples, B = 1, chunk_size 2,621,440) and a training-sized batch (16 rows of 2 s = 88,200 samples), offline
model, mix-phase.

Arms, each warmed up, alternated round by round (so drift lands on every arm alike) and timed with a host clock around work
that ends in a device synchronise -- arm (c) does host work, so device events alone would not see it:
    forward            (a) the four stems
    forward+score      (b) the stems, then scoring.score against targets that are on the device already
    forward+d2h+numpy  (c) what the package did before: the stems copied to the host and evaluation.global_sdr per target
    score              scoring.score alone on stems and targets that are already there (HIP events)
What matters is (b) - (a) against (c) - (a).  The accumulate kernel's own time comes from the library's event profiler
(xsq_profile_*: score_moments, score_combine, score_finalise) in calls of their own; its rate is the bytes the algorithm needs,
2 tensors x 4 stems x B x 2 channels x N x 4 bytes, over that time, printed beside the 6.29 TB/s a float4 copy reaches on this
part and the 8 TB/s of the HBM's specification.  ``working_set_mb`` against the 256 MiB Infinity Cache says where the
kernel reads from: the track's 677 MB cannot sit in it, the batch's 90 MB can (the estimates were written just before).

One JSON line per (shape, arm), appended to --out as well.

    python tools/score_bench.py [--rounds 7] [--iters 3] [--out profiles/score_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

TRACK_SAMPLES = 10_584_000
CHUNK = 2_621_440
SHAPES = {"track240s": (1, TRACK_SAMPLES), "rows16x2s": (16, 88_200)}
HBM_COPY_TBS, HBM_SPEC_TBS, INFINITY_CACHE_MB = 6.29, 8.0, 256 * 1.048576


def host_timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


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
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "score_bench.jsonl"))
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.evaluation import global_sdr
    from xumx_slicq_amd.scoring import TrackScorer, score
    from xumx_slicq_amd.separator import Separator, seeded_separator
    from xumx_slicq_amd.synth import synth_audio
    dev = torch.device("cuda", 0)
    sep = seeded_separator(realtime=False, wiener=False, device=dev, chunk_size=CHUNK)
    lines = []
    for shape in args.shapes:
        B, N = SHAPES[shape]
        x = synth_audio(N, seed=20260101, nb_samples=B).to(dev)
        # targets: seeded stems of the same size, in Separator.sources order; what they are does not change the work
        y = torch.stack([0.25 * synth_audio(N, seed=20260200 + k, nb_samples=B) for k in range(4)]).to(dev)
        y_host = [y[k].cpu().numpy() for k in range(4)]

        def parent():
            est = sep(x).cpu().numpy()
            return [[global_sdr(y_host[k][b].T, est[k, b].T) for b in range(B)] for k in range(4)]

        est0 = sep(x)
        scorer = TrackScorer(B, N, sample_rate=44100.0, device=dev)

        def score_only():
            scorer.position = scorer._covered = scorer._scored = 0
            return scorer.add(est0, y)

        arms = {"forward": (host_timed, lambda: sep(x)), "forward+score": (host_timed, lambda: score(sep(x), y)),
                "forward+d2h+numpy": (host_timed, parent), "score": (event_timed, lambda: score(est0, y)),
                "accumulate": (event_timed, score_only)}
        for timer, fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # the two routes must tell the same story before either is timed
        dev_glob = score(est0, y)["targets"]
        host_glob = parent()
        worst = max(abs(dev_glob[name]["sdr_global"][b] - host_glob[k][b]) for k, name in enumerate(Separator.sources) for b in range(B))
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, (timer, fn) in arms.items():
                times[name].append(timer(fn, 1 if name == "forward+d2h+numpy" else args.iters))
        _lib.profile_reset()
        _lib.profile_enable(True)
        for _ in range(args.rounds):
            score(est0, y)
        torch.cuda.synchronize()
        kern = {k: v[0] / max(v[1], 1) for k, v in _lib.profile_read().items() if k.startswith("score_")}
        _lib.profile_enable(False)
        nbytes = 2 * 4 * B * 2 * N * 4
        med = {name: float(np.median(t)) for name, t in times.items()}
        for name, t in times.items():
            t = np.array(t)
            line = {"tool": "score_bench", "shape": shape, "B": B, "samples": N, "arm": name, "rounds": args.rounds,
                    "clock": "hip-events" if arms[name][0] is event_timed else "host+synchronise",
                    "ms_median": round(med[name], 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                    "ms_over_forward": round(med[name] - med["forward"], 4) if name.startswith("forward") else None}
            if name == "accumulate":
                ms = kern.get("score_moments")
                line.update({"kernels_ms": {k: round(v, 5) for k, v in sorted(kern.items())}, "bytes": nbytes,
                             "working_set_mb": round(nbytes / 1e6, 1), "fits_infinity_cache": nbytes / 1e6 < INFINITY_CACHE_MB,
                             "score_moments_tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3) if ms else None,
                             "hbm_copy_tb_per_s": HBM_COPY_TBS, "hbm_spec_tb_per_s": HBM_SPEC_TBS,
                             "global_sdr_device_vs_numpy_max_abs_db": worst})
            lines.append(line)
            print(json.dumps(line), flush=True)
        del x, y, y_host, est0, scorer
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
