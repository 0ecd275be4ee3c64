"""Time Separator.forward_overlapped on the bench shape: one seeded 240 s stereo track (10,584,000 samples), the offline
model, mix-phase and Wiener-EM, chunk_size 2,621,440, the default segments (10.0 s hops, 0.1 s overlap: 22 segments that
process 1.009 x the track's samples).

Arms, each warmed up and timed with HIP events on the caller's stream, alternated round by round (so drift lands on
every arm alike):
    forward              the hard-joined chunks (what the overlapped result costs extra is read against this)
    loop                 the segment loop spelled in Python over Separator.forward, every segment multiplied by its whole
                         fade window and added into a zeroed result, as separate_sources of cadenza/enhance.py does: what a
                         caller had before forward_overlapped -- the baseline
    fallback             the package's own definition loop (separator.overlapped_loop: fades on the shared samples only)
    forward_overlapped   one native call
One JSON line per (mode, arm): median / min / max milliseconds over the rounds and the ratio to `forward` and to `loop`.
The forward_overlapped line also carries the time of its xsq_crossfade_place launches from the library's event profiler
(one more call, profiler on), their share of the call, and the kernel's achieved bytes/s -- scratch read once, result
written once, the cross-pass heads read back -- against the 6.29 TB/s float4-copy rate of an MI355X.

    python tools/overlap_bench.py [--rounds 7] [--iters 3] [--modes phasemix wiener] [--out FILE]
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
SEGMENT, OVERLAP = 10.0, 0.1
COPY_GBS = 6290.0


def reference_style_loop(sep, x, chunk_len, ov):
    from xumx_slicq_amd.separator import fade_weights, segments
    final = torch.zeros(4, x.shape[0], x.shape[1], x.shape[-1], device=x.device)
    w_in, w_out = fade_weights(ov, x.device)
    for start, n, fi, fo in segments(x.shape[-1], chunk_len, ov):
        w = torch.ones(n, device=x.device)
        if fi:
            w[:fi] = w_in
        if fo:
            w[n - fo:] = w_out
        final[..., start:start + n] += sep(x[..., start:start + n]) * w
    return final


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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", nargs="+", default=["phasemix", "wiener"], choices=["phasemix", "wiener"])
    ap.add_argument("--samples", type=int, default=TRACK_SAMPLES)
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.separator import overlapped_loop, seeded_separator, segment_lengths, segments
    from xumx_slicq_amd.synth import synth_audio
    assert torch.cuda.is_available(), "overlap_bench needs the GPU: a timing taken elsewhere says nothing"
    dev = torch.device("cuda", 0)
    N = args.samples
    x = synth_audio(N, seed=20260101).to(dev)
    chunk_len, ov = segment_lengths(44100.0, SEGMENT, OVERLAP, CHUNK)
    segs = segments(N, chunk_len, ov)
    processed = sum(s[1] for s in segs) / N
    lines = []
    for mode in args.modes:
        sep = seeded_separator(realtime=False, wiener=(mode == "wiener"), device=dev, chunk_size=CHUNK)
        table = {
            "forward": lambda t: sep(t),
            "loop": lambda t: reference_style_loop(sep, t, chunk_len, ov),
            "fallback": lambda t: overlapped_loop(sep.forward, t, chunk_len, ov),
            "forward_overlapped": lambda t: sep.forward_overlapped(t, SEGMENT, OVERLAP),
        }
        outs = {}
        for name, fn in table.items():              # warm-up: caches, workspaces, plans of every arm
            for _ in range(args.warmup):
                out = fn(x)
            torch.cuda.synchronize()
            outs[name] = out
        # the arms compute the same thing: the native call against the package's loop, and the whole-window loop near it
        same = bool(torch.equal(outs["forward_overlapped"], outs["fallback"]))
        loop_diff = float((outs["forward_overlapped"] - outs["loop"]).abs().max())
        outs.clear()
        del out
        times = {name: [] for name in table}
        for _ in range(args.rounds):
            for name, fn in table.items():
                times[name].append(time_once(fn, x, args.iters))
        _lib.profile_reset()
        _lib.profile_enable(True)
        table["forward_overlapped"](x)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        place_ms, launches = prof.get("crossfade_place", (0.0, 0))
        # rows x (scratch read + result written + the heads of the later passes read back) x 4 bytes
        place_bytes = 8 * (sum(s[1] for s in segs) + N + ov * max(0, launches - 1)) * 4
        med = {name: float(np.median(t)) for name, t in times.items()}
        for name in table:
            t = np.array(times[name])
            line = {"tool": "overlap_bench", "mode": mode, "arm": name, "samples": N, "chunk_size": CHUNK, "segment": SEGMENT,
                    "overlap": OVERLAP, "segments": len(segs), "processed_ratio": round(processed, 4), "rounds": args.rounds,
                    "iters": args.iters, "ms_median": round(med[name], 4), "ms_min": round(float(t.min()), 4),
                    "ms_max": round(float(t.max()), 4), "vs_forward": round(med[name] / med["forward"], 4),
                    "vs_loop": round(med[name] / med["loop"], 4)}
            if name == "forward_overlapped":
                line.update({"bitwise_equal_to_fallback": same, "max_abs_diff_to_loop": loop_diff,
                             "crossfade_place_ms": round(place_ms, 4), "crossfade_place_launches": launches,
                             "crossfade_place_share_of_profiled_call": round(place_ms / max(sum(v[0] for v in prof.values()), 1e-9), 4),
                             "crossfade_place_bytes": place_bytes,
                             "crossfade_place_gbs": round(place_bytes / max(place_ms, 1e-9) / 1e6, 1),
                             "crossfade_place_vs_copy_rate": round(place_bytes / max(place_ms, 1e-9) / 1e6 / COPY_GBS, 4)})
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del sep, table
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
