"""What the mirrored synthesis of the bands across DC (``dc_twins=True``, csrc/dc_twins.h) costs, measured on the device.

Three measurements, one JSON line each, appended to profiles/dc_twins_bench.jsonl (``--out``):

  inverse       the inverse transform of ``bark, 56, 32.9`` (plan K) and ``bark, 96, 32.9`` on a seeded 30 s stereo signal
                (1,323,000 samples): the whole call by HIP events on the caller's stream, and the twin kernel's own time from the
                library's event profiler (xsq_profile_*, "twin_synthesis") in calls of their own -- medians of ``--rounds``
                rounds, the plans alternated round by round.
  search-step   one ``TrackEvaluator(..., dc_twins=True).oracle`` round on ``bark, 28, 32.9`` (plan T) over two seeded 30 s tracks
                (host clock around work that ends in a device-to-host read; builds and frees its own plan).
  headline      ``bench.py --gpus 1 --steps K --warmup W`` of this tree and of a built checkout of the parent commit
                (``--parent DIR``), as child processes alternated in one session: the value of each run and the medians.

Nothing is asserted: the lines say what was measured.

    python tools/dc_twins_bench.py [--parent DIR] [--rounds 7] [--bench-pairs 2] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

INVERSE_PLANS = {"K": ("bark", 56, 32.9), "bark96": ("bark", 96, 32.9)}
SEARCH_PLAN = ("bark", 28, 32.9)
SECONDS = 30


def inverse_lines(rounds, iters):
    from xumx_slicq_amd import _lib
    from xumx_slicq_amd.synth import synth_audio
    from xumx_slicq_amd.transforms import NSGTBase, make_filterbanks
    n = SECONDS * 44100
    x = synth_audio(n, seed=20261021).cuda()                                              # (1, 2, n)
    banks, coefs = {}, {}
    for name, cfg in INVERSE_PLANS.items():
        base = NSGTBase(*cfg, device="cuda", dc_twins=True)
        banks[name] = (base, *make_filterbanks(base))
        coefs[name] = banks[name][1](x)
        for _ in range(3):                                                               # warm-up: code objects, rocFFT plans
            banks[name][2](coefs[name], n)
    torch.cuda.synchronize()
    whole = {k: [] for k in banks}
    twin = {k: [] for k in banks}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, (base, enc, dec) in banks.items():                                      # the plans alternate inside a round
            a.record()
            for _ in range(iters):
                dec(coefs[name], n)
            b.record()
            b.synchronize()
            whole[name].append(a.elapsed_time(b) / iters)
            _lib.profile_enable(True)                                                     # the kernel's own time: calls of their own
            _lib.profile_reset()
            for _ in range(iters):
                dec(coefs[name], n)
            torch.cuda.synchronize()
            prof = _lib.profile_read()
            _lib.profile_enable(False)
            ms, count = prof["twin_synthesis"]
            assert count == iters, prof
            twin[name].append(ms / count)
    lines = []
    for name, (base, enc, dec) in banks.items():
        p = base.plan
        S = p.num_slices(n)
        lines.append({"tool": "dc_twins_bench", "what": "inverse", "plan": list(INVERSE_PLANS[name]), "L": p.L, "samples": n, "rows": 2 * S,
                      "landing_entries": sum(len(t[1]) for t in p.twins), "rounds": rounds, "iters": iters, "clock": "HIP events",
                      "call_ms_median": round(float(np.median(whole[name])), 4), "call_ms_min": round(min(whole[name]), 4),
                      "call_ms_max": round(max(whole[name]), 4), "twin_synthesis_ms_median": round(float(np.median(twin[name])), 5),
                      "twin_share_of_call": round(float(np.median(twin[name]) / np.median(whole[name])), 5)})
        base.nsgt.close()
    return lines


def search_line(rounds):
    from xumx_slicq_amd.data import DeviceDataset
    from xumx_slicq_amd.slicqfinder import TrackEvaluator
    from xumx_slicq_amd.synth import synth_audio
    n = SECONDS * 44100
    tracks = [{s: (g * synth_audio(n, seed=20260400 + 10 * t + j)[0]).numpy()
               for j, (s, g) in enumerate(zip(DeviceDataset.sources, (0.5, 0.35, 0.25, 0.4)))} for t in range(2)]
    ds = DeviceDataset.from_arrays(tracks, storage="fp32", device="cuda")
    ev = TrackEvaluator(ds, dc_twins=True)
    scale, bins, fmin = SEARCH_PLAN
    ev.oracle(scale, fmin, bins)                                                          # warm-up
    step = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sdr = ev.oracle(scale, fmin, bins)
        step.append((time.perf_counter() - t0) * 1e3)
    return {"tool": "dc_twins_bench", "what": "search-step", "plan": list(SEARCH_PLAN), "tracks": len(ds), "samples": n, "arm": "TrackEvaluator.oracle",
            "rounds": rounds, "clock": "host, ends in a device-to-host read", "ms_median": round(float(np.median(step)), 3), "ms_min": round(min(step), 3),
            "ms_max": round(max(step), 3), "sdr": [round(float(v), 4) for v in sdr], "refusals": len(ev.refusals)}


def headline_line(parent, pairs, steps, warmup):
    trees = {"tree": ROOT, "parent": os.path.abspath(parent)}
    runs = {k: [] for k in trees}
    for _ in range(pairs):
        for name, d in trees.items():                                                     # alternated: drift lands on both alike
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=d, check=True,
                               capture_output=True, text=True, timeout=900)
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            runs[name].append(res["value"])
            print(f"bench.py in {name}: {res['value']} {res.get('unit', '')}", flush=True)
    return {"tool": "dc_twins_bench", "what": "headline", "cmd": f"bench.py --gpus 1 --steps {steps} --warmup {warmup}", "unit": "x real-time", "pairs": pairs,
            "order": "tree, parent, tree, parent, ...", "tree": runs["tree"], "parent": runs["parent"],
            "tree_median": float(np.median(runs["tree"])), "parent_median": float(np.median(runs["parent"])),
            "tree_over_parent": round(float(np.median(runs["tree"]) / np.median(runs["parent"])), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (omit: no headline line)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--bench-pairs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_twins_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dc_twins_bench: needs an MI355X (no CPU fallback, no CPU numbers)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(lines):                                                                      # as soon as measured
        with open(args.out, "a") as f:
            for line in lines:
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")

    emit(inverse_lines(args.rounds, args.iters))
    emit([search_line(args.rounds)])
    if args.parent:
        emit([headline_line(args.parent, args.bench_pairs, args.steps, args.warmup)])


if __name__ == "__main__":
    main()
