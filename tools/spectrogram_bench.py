"""Time the sliCQT spectrogram against what it replaces, on the bench track: one seeded 240 s stereo track (10,584,000 samples,
B = 1), Bark-262, width 2560.

Arms, each warmed up, alternated round by round (so drift lands on every arm alike); medians over the rounds:
    forward               (a) the forward transform alone                                                   HIP events
    forward+picture       (b) visualization.spectrogram: forward, dB pass, radix select, raster             HIP events
    forward+torch         (c) the same picture composed from torch ops on the device: views of the arena, strided adds, abs,
                              log10, mean, one sort for the quantile, a gather + max for the pooling         HIP events
    forward+d2h+numpy     (d) forward, the full-resolution dB values copied to the host, numpy partition and reduceat
                                                                                                             host clock + synchronise
    picture               the picture path alone on an arena that is already there                           HIP events
What matters is (b) - (a) against (c) - (a) and (d) - (a).  The kernels' own times come from the library's event profiler
(xsq_profile_*: spec_db, spec_hist, spec_pick, spec_raster) in calls of their own; their rates are the bytes the algorithm
needs over that time, beside the rate of a device-to-device copy of the arena measured in the same process (read + write
bytes over its time) and the 6.29 TB/s float4 copy rate tools/score_bench.py quotes.

The picture path rasters the MATERIALISED dB array.  The other variant -- a raster kernel that recomputes dB from the arena while
it pools -- was measured with this tool on the same track before it was dropped (the lines with "picture-recompute" and
"spec_raster_arena" in profiles/spectrogram_bench.jsonl): the same bits, 0.111 ms against 0.087 ms.

One JSON line per arm and per kernel, appended to --out as well.

    python tools/spectrogram_bench.py [--rounds 7] [--iters 3] [--out profiles/spectrogram_bench.jsonl]
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
WIDTH = 2560
HBM_COPY_TBS, HBM_SPEC_TBS = 6.29, 8.0


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
    ap.add_argument("--samples", type=int, default=TRACK_SAMPLES)
    ap.add_argument("--width", type=int, default=WIDTH)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "spectrogram_bench.jsonl"))
    args = ap.parse_args()

    from xumx_slicq_amd import _lib
    from xumx_slicq_amd import visualization as vis
    from xumx_slicq_amd.synth import synth_audio
    from xumx_slicq_amd.transforms import NSGTBase
    dev = torch.device("cuda", 0)
    base = NSGTBase("bark", 262, 32.9, device=dev)
    eng, plan = base.nsgt, base.plan
    n, W = args.samples, args.width
    x = synth_audio(n, seed=20260101, nb_samples=1).to(dev)
    S = plan.num_slices(n)
    geo = vis._Geometry(plan, n, S, 1, False)
    arena0, _, _ = eng.forward(x)
    q = 0.999
    k_lo, k_hi, t = vis.quantile_ranks(geo.per_item, q)

    # (c) tables of the torch composition, built once: per block the gather index of the pooling
    pools = []
    for N in geo.columns:
        lo, hi = vis.raster_ranges(N, W)
        span = int((hi - lo).max())
        idx = np.minimum(lo[:, None] + np.arange(span)[None, :], (hi - 1)[:, None])
        pools.append(torch.from_numpy(idx).to(dev))

    def picture_torch(arena):
        rows, vals = [], []
        for X, N, idx in zip(eng.table.views(arena, (1, 2), S), geo.columns, pools):
            c = torch.view_as_complex(X)                                   # (1, 2, F, S, T)
            h = c.shape[-1] // 2
            ola = (c[..., :-1, h:] + c[..., 1:, :h]).flatten(-2, -1)       # the cropped overlap-add: two terms at every point
            db = (20.0 * torch.log10(torch.abs(ola))).mean(dim=1)[..., :N]
            vals.append(db.reshape(-1))
            rows.append(db[..., idx].amax(dim=-1))
        v = torch.sort(torch.cat(vals)).values
        lo_hi = torch.stack([v[k_lo], v[k_hi]]).cpu().numpy().astype(np.float64)
        return torch.cat(rows, dim=1), vis.quantile_lerp(lo_hi[0], lo_hi[1], t)

    def picture_numpy(arena):
        blocks = [d.cpu().numpy() for d in geo.views(vis._db(geo, arena))]
        allv = np.concatenate([d.reshape(-1) for d in blocks])
        part = np.partition(allv, (k_lo, k_hi))
        rows = [np.maximum.reduceat(d, vis.raster_ranges(d.shape[-1], W)[0], axis=-1) for d in blocks]
        return np.concatenate(rows, axis=1), vis.quantile_lerp(part[k_lo], part[k_hi], t)

    def picture(arena):
        db = vis._db(geo, arena)
        img = vis._raster(geo, db, W)
        stats, tt = vis._order_stats(geo.F, geo.N, db, 1, q)
        return img, vis.quantile_lerp(stats[0, 0], stats[0, 1], tt)

    # the three routes must draw the same picture before any of them is timed
    sp = vis.spectrogram(x, base, width=W)
    img_t, vmax_t = picture_torch(arena0)
    img_n, vmax_n = picture_numpy(arena0)
    img_d = sp.image.cpu().numpy()
    fin = np.isfinite(img_d)
    agree = {"numpy_image_bitwise": bool(np.array_equal(img_n.view(np.uint32), img_d.view(np.uint32))), "numpy_vmax_equal": bool(vmax_n == sp.vmax[0]),
             "torch_image_max_abs_db": float(np.abs(img_t.cpu().numpy()[fin] - img_d[fin]).max()), "torch_vmax_abs_db": float(abs(vmax_t - sp.vmax[0]))}
    print(json.dumps({"tool": "spectrogram_bench", "agreement": agree}), flush=True)

    arms = {"forward": (event_timed, lambda: eng.forward(x)),
            "forward+picture": (event_timed, lambda: vis.spectrogram(x, base, width=W)),
            "forward+torch": (event_timed, lambda: picture_torch(eng.forward(x)[0])),
            "forward+d2h+numpy": (host_timed, lambda: picture_numpy(eng.forward(x)[0])),
            "picture": (event_timed, lambda: picture(arena0))}
    for timer, fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, (timer, fn) in arms.items():
            times[name].append(timer(fn, 1 if name == "forward+d2h+numpy" else args.iters))

    # kernels: the library's profiler, and a copy of the arena as the yardstick
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(args.rounds):
        picture(arena0)
    torch.cuda.synchronize()
    kern = {k: v[0] / max(v[1], 1) for k, v in _lib.profile_read().items() if k.startswith("spec_")}
    _lib.profile_enable(False)
    dst = torch.empty_like(arena0)
    for _ in range(args.warmup):
        dst.copy_(arena0)
    copy_ms = float(np.median([event_timed(lambda: dst.copy_(arena0), args.iters) for _ in range(args.rounds)]))
    del dst
    arena_bytes = arena0.numel() * 4
    db_bytes = geo.per_item * 4
    img_bytes = plan.nbands * W * 4
    # bytes the algorithm needs: the dB pass reads the slices that contribute and writes the dB values; a histogram pass reads them
    read_share = sum(F * 2 * N for F, N in zip(geo.F.tolist(), geo.columns)) / sum(F * S * T for F, T in zip(geo.F.tolist(), geo.T.tolist()))
    needs = {"spec_db": arena_bytes * read_share + db_bytes, "spec_hist": db_bytes, "spec_raster": db_bytes + img_bytes, "spec_pick": 2 * 256 * 4}
    med = {name: float(np.median(v)) for name, v in times.items()}
    lines = []
    for name, v in times.items():
        v = np.array(v)
        lines.append({"tool": "spectrogram_bench", "samples": n, "width": W, "slices": S, "arm": name, "rounds": args.rounds,
                      "clock": "hip-events" if arms[name][0] is event_timed else "host+synchronise", "ms_median": round(med[name], 4),
                      "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                      "ms_over_forward": round(med[name] - med["forward"], 4) if name.startswith("forward") else None})
    for name, ms in sorted(kern.items()):
        nb = needs.get(name)
        lines.append({"tool": "spectrogram_bench", "samples": n, "width": W, "kernel": name, "ms_per_launch": round(ms, 5),
                      "bytes": int(nb) if nb else None, "tb_per_s": round(nb / (ms * 1e-3) / 1e12, 3) if nb and ms else None})
    lines.append({"tool": "spectrogram_bench", "samples": n, "yardstick": "device copy of the arena (torch copy_, read + write)", "arena_mb": round(arena_bytes / 1e6, 1),
                  "db_mb": round(db_bytes / 1e6, 1), "image_mb": round(img_bytes / 1e6, 2), "ms": round(copy_ms, 4),
                  "tb_per_s": round(2 * arena_bytes / (copy_ms * 1e-3) / 1e12, 3), "float4_copy_tb_per_s_score_bench": HBM_COPY_TBS,
                  "hbm_spec_tb_per_s": HBM_SPEC_TBS, "agreement": agree})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
