"""Time the front end's resampler (csrc/resample.hip) on a 240 s stereo track at 48 and 96 kHz -> 44.1 kHz with HIP
events, next to the same filter applied as torchaudio applies it on a GPU (pad + torch.nn.functional.conv1d with stride
o + reorder, the full n x (2*width + o) table), and print both against the HBM bound of the kernel's traffic
(rows x (L + L') x 4 bytes at 6.29 TB/s, the float4-copy rate of an MI355X).  One JSON line per case.

    python tools/resample_bench.py [--seconds 240] [--iters 50] [--rates 48000 96000]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from xumx_slicq_amd.resample import filter_taps, resample, resample_table  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def conv1d_form(orig, new, device):
    """torchaudio's formulation: the full table as conv1d weights (n, 1, 2*width + o)."""
    tab = resample_table(orig, new)
    o, n, w = tab.orig, tab.new, tab.width
    K = filter_taps(np.arange(n)[:, None], np.arange(2 * w + o)[None, :], o, n)
    weight = torch.from_numpy(K).to(device)[:, None, :]

    def run(x):
        rows, L = x.shape
        xp = F.pad(x[:, None, :], (w, w + o))
        y = F.conv1d(xp, weight, stride=o)                                  # (rows, n, L // o + 1)
        return y.transpose(1, 2).reshape(rows, -1)[:, :tab.output_length(L)]
    return run


def time_ms(fn, x, iters):
    for _ in range(3):
        fn(x)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn(x)
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rates", type=int, nargs="+", default=[48000, 96000])
    ap.add_argument("--new", type=int, default=44100)
    ap.add_argument("--no-conv1d", action="store_true", help="time the HIP kernel only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    dev = torch.device("cuda", 0)
    for rate in args.rates:
        L = int(args.seconds * rate)
        x = torch.rand(2, L, device=dev) * 2 - 1
        hip = lambda v: resample(v, rate, args.new)                          # noqa: E731
        y = hip(x)
        Lo = y.shape[-1]
        bound_us = 2 * (L + Lo) * 4 / HBM_BYTES_PER_S * 1e6
        med, best = time_ms(hip, x, args.iters)
        rec = {"case": f"{rate}->{args.new}", "seconds": args.seconds, "rows": 2, "len_in": L, "len_out": Lo,
               "taps": resample_table(rate, args.new).span, "hbm_bound_us": round(bound_us, 1),
               "hip_us_median": round(med * 1e3, 1), "hip_us_best": round(best * 1e3, 1),
               "hip_of_bound": round(bound_us / (med * 1e3), 3)}
        if not args.no_conv1d:
            conv = conv1d_form(rate, args.new, dev)
            yc = conv(x)
            cmed, cbest = time_ms(conv, x, max(5, args.iters // 5))
            rec.update({"conv1d_us_median": round(cmed * 1e3, 1), "conv1d_us_best": round(cbest * 1e3, 1),
                        "conv1d_over_hip": round(cmed / med, 2),
                        "max_abs_diff_vs_conv1d": float((yc - y).abs().max()) if yc.shape == y.shape else None})
        print(json.dumps(rec), flush=True)
        del x, y


if __name__ == "__main__":
    main()
