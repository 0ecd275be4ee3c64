"""Time a steady-state step of a streaming session (Separator.stream) against the same step spelled through Separator.forward.

Per plan (the Bark-262 realtime model and the Mel-32 realtime model) and per hop_slices m (1, 2, 4, 8), both arms warmed up, timed
with HIP events on the caller's stream over `iters` consecutive steps, alternated round by round (so drift lands on both alike):
    native   one feed of m blocks (m * sllen / 2 samples) into a session in steady state: one ring write and one xsq_stream_step
    loop     the body of a steady-state step of separator.streamed_loop: Separator.forward on the sub-signal that gives the m
             blocks their context ((2 (m + back + ahead + 2) + 2) * sllen / 4 samples), the blocks copied out of its result --
             what a caller had before the session: the baseline
One JSON line per (plan, m): median / min / max milliseconds per step of both arms and their ratio, the audio a step emits and the
share of it the native step takes (the real-time budget), the session's state_bytes, whether the session's joined result over a
signal of 6 m + 16 blocks is bitwise Separator.forward of the whole (it is up to 64 slices; from 65 on the whole call's CDAE takes
its long-row kernels and the two differ in the last bits: the largest difference is recorded), and the native step's kernels from the library's event
profiler (one more run of `iters` steps, profiler on): the forward transform of the whole window -- context slices included, it is
recomputed every step -- beside the CDAE and the emission.

    python tools/stream_bench.py [--rounds 9] [--iters 20] [--hops 1 2 4 8] [--plans bark mel] [--out profiles/stream_bench.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

PLANS = {"bark": dict(), "mel": dict(fscale="mel", fbins=32, fmin=115.5)}
RATE = 44100.0


def timed(fn, iters):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--hops", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--plans", nargs="+", default=["bark", "mel"], choices=list(PLANS))
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.inference import stream_blocks
    from xumx_slicq_amd.separator import _loop_span, seeded_separator
    from xumx_slicq_amd.synth import synth_audio
    assert torch.cuda.is_available(), "stream_bench needs the GPU: a timing taken elsewhere says nothing"
    dev = torch.device("cuda", 0)
    lines = []
    for plan in args.plans:
        sep = seeded_separator(realtime=True, device=dev, **PLANS[plan])
        for m in args.hops:
            session = sep.stream(1, m)
            h, back, ahead = session.h, session.back, session.ahead
            per = 2 * h * m
            # both arms walk the same track round and round; a steady-state step of the loop, far from both ends
            x = synth_audio(per * (args.warmup + args.iters + 8), seed=20261019).to(dev)
            b0 = (back + 4) * m
            t0, t1 = _loop_span(b0, b0 + m + ahead, h, back, None)
            assert t0 > 0 and t1 <= x.shape[-1]
            out = torch.empty(4, 1, 2, per, device=dev)
            pos = [0]

            def native_step():
                p = pos[0]
                pos[0] = p + per if p + 2 * per <= x.shape[-1] else 0
                return session.feed(x[..., p:p + per])

            def loop_step():
                est = sep.forward(x[..., t0:t1])
                out[...] = est[..., b0 * 2 * h - t0:b0 * 2 * h - t0 + per]

            check = synth_audio(2 * h * (6 * m + 16) + 17, seed=7).to(dev)
            joined, whole = stream_blocks(check, sep, 4096, m), sep.forward(check)
            same, diff = bool(torch.equal(joined, whole)), float((joined - whole).abs().max())
            del joined, whole
            for _ in range(args.warmup):
                emitted = native_step()
                loop_step()
            torch.cuda.synchronize()
            assert emitted.shape[-1] == per, "the session is in steady state: every feed of m blocks releases one step"
            times = {"native": [], "loop": []}
            for _ in range(args.rounds):
                times["native"].append(timed(native_step, args.iters))
                times["loop"].append(timed(loop_step, args.iters))
            _lib.profile_reset()
            _lib.profile_enable(True)
            for _ in range(args.iters):
                native_step()
            torch.cuda.synchronize()
            prof = _lib.profile_read()
            _lib.profile_enable(False)
            med = {k: float(np.median(v)) for k, v in times.items()}
            audio_ms = per / RATE * 1e3
            kernels = {k: round(ms / args.iters * 1e3, 2) for k, (ms, _) in sorted(prof.items())}
            fwd_us = sum(v for k, v in kernels.items() if k.startswith(("slice_rfft", "slice_window", "rfft_L", "band_analysis")))
            line = {"tool": "stream_bench", "plan": plan, "model": "realtime", "hop_slices": m, "nb_samples": 1, "sllen": 4 * h,
                    "window_slices": m + back + ahead, "loop_samples": t1 - t0, "rounds": args.rounds, "iters": args.iters,
                    "native_ms_median": round(med["native"], 4), "native_ms_min": round(min(times["native"]), 4),
                    "native_ms_max": round(max(times["native"]), 4), "loop_ms_median": round(med["loop"], 4),
                    "loop_ms_min": round(min(times["loop"]), 4), "loop_ms_max": round(max(times["loop"]), 4),
                    "native_vs_loop": round(med["native"] / med["loop"], 4), "audio_ms_per_step": round(audio_ms, 3),
                    "native_share_of_realtime": round(med["native"] / audio_ms, 5), "latency_samples": session.latency_samples,
                    "state_bytes": session.state_bytes, "bitwise_equal_to_forward": same, "max_abs_diff_to_forward": diff,
                    "check_slices": 6 * m + 17,
                    "profiled_kernels_us_per_step": kernels, "profiled_forward_transform_us": round(fwd_us, 2),
                    "profiled_total_us": round(sum(kernels.values()), 2)}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
            del session
        del sep
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
