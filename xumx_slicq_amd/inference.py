"""Counterpart of /root/reference/xumx_slicq_v2/inference.py for the ROCm backend:
``separate`` (inference.py:14-33, same timing convention: wall time of the
``separator(audio)`` call only) and a small CLI (``python -m xumx_slicq_amd``)."""
from __future__ import annotations

import argparse
import time
import warnings
from pathlib import Path

import torch

from . import audio as xaudio
from .resample import Resample
from .separator import Separator, remix_gains, seeded_separator


def separate(audio, separator, rate=None, device=None):
    """inference.py:14-33: returns ({target: (nb_samples, 2, T)}, seconds)."""
    if rate is None:
        raise Exception("rate` must be provided.")
    if device:
        audio = audio.to(device)
    audio = xaudio.preprocess_audio(audio, rate, separator.sample_rate)
    torch.cuda.synchronize(audio.device)
    start_time = time.time()
    estimates = separator(audio)
    torch.cuda.synchronize(audio.device)
    time_delta = time.time() - start_time
    return separator.to_dict(estimates), time_delta


def parse_remix_spec(spec: str):
    """``--remix NAME:SPEC`` -> (NAME, gain row in Separator.sources order).  SPEC is a comma-separated list of
    target=gain; targets not named keep gain 1.0 (``karaoke:vocals=0``, ``instrumental:vocals=0,drums=0.5``).
    ValueError for a missing or unusable NAME, an unknown target, a target named twice or a gain that is not a finite
    number.  Host only."""
    name, sep, body = spec.partition(":")
    name = name.strip()
    if not sep or not name or name in (".", "..") or any(c in name for c in "/\\\0"):
        raise ValueError(f"--remix wants NAME:SPEC with a file name NAME, got {spec!r}")
    gains = {}
    for item in filter(None, (x.strip() for x in body.split(","))):
        target, eq, value = item.partition("=")
        target = target.strip()
        if not eq:
            raise ValueError(f"--remix {spec!r}: {item!r} is not target=gain")
        if target in gains:
            raise ValueError(f"--remix {spec!r}: target {target!r} named twice")
        try:
            gains[target] = float(value)
        except ValueError:
            raise ValueError(f"--remix {spec!r}: gain {value!r} of {target!r} is not a number") from None
    return name, remix_gains(gains)[0].tolist()


def parse_remix_specs(specs):
    """The repeated ``--remix`` options -> (names, (R, 4) gains); None when there are none.  At most four, names unique."""
    if not specs:
        return None
    if len(specs) > 4:
        raise ValueError(f"at most four --remix mixes per run (got {len(specs)})")
    parsed = [parse_remix_spec(s) for s in specs]
    names = [n for n, _ in parsed]
    if len(set(names)) != len(names):
        raise ValueError(f"--remix names must be unique: {names}")
    return names, remix_gains([row for _, row in parsed])


class _PinnedPool:
    """Pinned host buffers handed round between the pipeline's threads (hipHostMalloc of a 339 MB stem block costs more
    than demixing the track: buffers are allocated once per size class and reused)."""

    def __init__(self):
        import queue
        self._free = queue.Queue()
        self._count = 0

    def take(self, numel: int, limit: int):
        """A pinned fp32 buffer of >= numel elements; blocks when `limit` buffers are out and none is free."""
        import queue
        while True:
            try:
                buf = self._free.get(block=self._count >= limit)
            except queue.Empty:
                buf = None
            if buf is None:
                self._count += 1
                return torch.empty(numel, dtype=torch.float32, pin_memory=True)      # (allocated pinned: no pageable twin, no copy)
            if buf.numel() >= numel:
                return buf
            self._count -= 1          # too small for this track: drop it, allocate a larger one
            del buf

    def give(self, buf):
        self._free.put(buf)


_POOLS: dict = {}        # process-wide pinned staging pools of demix_directory


def demix_directory(separator, wavs, out_dir, device="cuda", readers: int = 3, writers: int = 4, depth: int = 3, quiet=False,
                    remix=None, overlapped=None):
    """The CLI's loop (inference.py:118-146) as a pipeline over the tracks: decode -> pinned host buffer (reader threads) |
    H2D on a copy stream | resampling to the model's rate on the GPU where the file's rate differs (preprocess_audio,
    data.py:148-156) | ``separator(audio)`` | channel interleave on the GPU (the wav payload layout, so the host never
    transposes 339 MB per track) | D2H into a pinned buffer on a second copy stream | header + payload written by writer
    threads.  At ~5 ms of GPU time per 240 s track the loop is bound by PCIe and file I/O; the stages of consecutive
    tracks overlap.  Stems are written at ``separator.sample_rate`` (inference.py:135-142).  ``remix`` = (names, (R, 4)
    gains) from ``parse_remix_specs``: ``separator.remix`` runs instead and writes <NAME>.wav per mix in place of the four
    stems.  ``overlapped`` = (segment seconds, overlap fraction): ``separator.forward_overlapped`` runs instead of
    ``separator(audio)`` (not together with ``remix``).  Returns [(name, audio seconds, separator milliseconds by HIP
    events)] in input order."""
    if remix is not None and overlapped is not None:
        raise ValueError("an overlapped remix is not built: remix or overlapped, not both")
    import queue
    import threading
    from concurrent.futures import ThreadPoolExecutor

    dev = torch.device(device)
    out_dir = Path(out_dir)
    names = list(separator.sources) + (["residual"] if getattr(separator, "residual", False) else []) if remix is None else list(remix[0])
    model_rate = int(float(separator.sample_rate))
    # the staging buffers outlive the call (page-locking a 339 MB block costs more than demixing the track it carries)
    pool_in, pool_out = _POOLS.setdefault("in", _PinnedPool()), _POOLS.setdefault("out", _PinnedPool())
    copy_in, copy_out = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream(dev)
    results, errors = {}, []
    wq: "queue.Queue" = queue.Queue()

    def read(path):
        keep = []

        def take(numel):
            keep.append(pool_in.take(numel, depth + readers))
            return keep[0]
        view, rate = xaudio.load_audio_into(str(path), take)        # (2, N) float32 in the pinned buffer, decoded in one pass
        return path, view, keep[0], rate

    lock = threading.Lock()

    def writer():
        # one job = ONE stem of one track: the four stems of a track go out on four threads at once (a track's last write is what
        # the end of a run waits for); the track's pinned buffer returns to the pool with its last stem
        while True:
            job = wq.get()
            if job is None:
                return
            path, host, buf, done, t0, t1, rate, n, k, left = job
            try:
                done.synchronize()
                target_dir = out_dir / path.stem
                target_dir.mkdir(parents=True, exist_ok=True)
                xaudio.save_wav_float_interleaved(str(target_dir / f"{names[k]}.wav"), host[k], model_rate)
            except Exception as e:                                   # noqa: BLE001 -- reported after the loop
                errors.append((str(path), e))
            finally:
                with lock:
                    left[0] -= 1
                    last = left[0] == 0
                if last:
                    results[str(path)] = (path.name, n / rate, t0.elapsed_time(t1))
                    pool_out.give(buf)

    threads = [threading.Thread(target=writer, daemon=True) for _ in range(writers)]
    for t in threads:
        t.start()
    wavs = [Path(w) for w in wavs]
    with ThreadPoolExecutor(max_workers=readers) as ex:
        pending = [ex.submit(read, w) for w in wavs]
        for fut in pending:
            path, view, buf_in, rate = fut.result()
            n = view.shape[-1]
            with torch.cuda.stream(copy_in):
                x = view.to(dev, non_blocking=True)[None]            # (1, 2, N)
                up = torch.cuda.Event()
                up.record(copy_in)
            main.wait_event(up)
            x.record_stream(main)
            if rate != model_rate:                                   # (1, 2, N'), on the main stream, outside the timed region
                warnings.warn("resample to model sample rate")
                x = Resample(rate, model_rate, resampling_method="sinc_interpolation")(x)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(main)
            if overlapped is not None:
                est = separator.forward_overlapped(x, *overlapped)
            else:
                est = separator(x) if remix is None else separator.remix(x, remix[1])      # (4 | R, 1, 2, N')
            t1.record(main)
            inter = est[:, 0].transpose(1, 2).contiguous()           # (4 | 5 | R, N', 2): the wav payload of each target
            ready = torch.cuda.Event()
            ready.record(main)
            buf_out = pool_out.take(inter.numel(), depth + writers)
            host = buf_out[:inter.numel()].view(inter.shape)
            with torch.cuda.stream(copy_out):
                copy_out.wait_event(ready)
                host.copy_(inter, non_blocking=True)
                inter.record_stream(copy_out)
                done = torch.cuda.Event()
                done.record(copy_out)
            up.synchronize()                                         # the input buffer may be refilled once its upload is over
            pool_in.give(buf_in)
            left = [len(names)]
            for k in range(len(names)):
                wq.put((path, host, buf_out, done, t0, t1, rate, n, k, left))
    for _ in threads:
        wq.put(None)
    for t in threads:
        t.join()
    if errors:
        raise RuntimeError("demix_directory: %d track(s) failed, first: %s: %r" % (len(errors), errors[0][0], errors[0][1]))
    out = [results[str(w)] for w in wavs]
    if not quiet:
        for name, secs, ms in out:
            print(f"{name}: {secs:.1f} s demixed in {ms:.1f} ms")
    return out


def _remix_one(audio, separator, rate, device, remix):
    """``separate`` with ``separator.remix``: ({name: (nb_samples, 2, T)}, seconds)."""
    if device:
        audio = audio.to(device)
    audio = xaudio.preprocess_audio(audio, rate, separator.sample_rate)
    torch.cuda.synchronize(audio.device)
    start_time = time.time()
    mixes = separator.remix(audio, remix[1])
    torch.cuda.synchronize(audio.device)
    return dict(zip(remix[0], mixes)), time.time() - start_time


def _overlapped_one(audio, separator, rate, device, overlapped):
    """``separate`` with ``separator.forward_overlapped``: ({target: (nb_samples, 2, T)}, seconds)."""
    if device:
        audio = audio.to(device)
    audio = xaudio.preprocess_audio(audio, rate, separator.sample_rate)
    torch.cuda.synchronize(audio.device)
    start_time = time.time()
    estimates = separator.forward_overlapped(audio, *overlapped)
    torch.cuda.synchronize(audio.device)
    return separator.to_dict(estimates), time.time() - start_time


def stream_blocks(audio, separator, block_samples: int, hop_slices: int = 1):
    """``audio`` (nb_samples, 2, N) pushed through a ``Separator.stream`` session in blocks of ``block_samples``: (4, nb_samples, 2, N),
    the returns of every ``feed`` and of ``flush`` joined."""
    session = separator.stream(audio.shape[0], hop_slices)
    parts = [session.feed(audio[..., p:p + block_samples]) for p in range(0, audio.shape[-1], block_samples)]
    return torch.cat(parts + [session.flush()], dim=-1)


def _stream_one(audio, separator, rate, device, block_samples, hop_slices):
    """``separate`` through a streaming session: ({target: (nb_samples, 2, T)}, seconds)."""
    if device:
        audio = audio.to(device)
    audio = xaudio.preprocess_audio(audio, rate, separator.sample_rate)
    torch.cuda.synchronize(audio.device)
    start_time = time.time()
    estimates = stream_blocks(audio, separator, block_samples, hop_slices)
    torch.cuda.synchronize(audio.device)
    return separator.to_dict(estimates), time.time() - start_time


def overlapped_option(args):
    """(segment, overlap) when --segment or --overlap was given (the other takes its default), else None."""
    if args.segment is None and args.overlap is None:
        return None
    return (10.0 if args.segment is None else args.segment, 0.1 if args.overlap is None else args.overlap)


def parse_args(p: argparse.ArgumentParser, argv=None):
    """``p.parse_args`` plus the checks between options.  Host only."""
    args = p.parse_args(argv)
    if args.niter is not None:
        if args.niter < 0:
            p.error(f"--niter {args.niter}: the iteration count is >= 0")
        if args.realtime:
            p.error("--niter counts the EM iterations of the offline model's Wiener filter; --realtime is mix-phase and has none")
    for opt in ("softmask", "residual"):
        if getattr(args, opt) and args.realtime:
            p.error(f"--{opt} is an option of the offline model's Wiener filter; --realtime is mix-phase and has none")
    if args.residual and args.remix:
        p.error("--residual writes residual.wav beside the four stems; --remix weights the four targets and has no column for it")
    if args.segment is not None or args.overlap is not None:
        if args.remix:
            p.error("--segment / --overlap write the four stems from overlapped, cross-faded segments; an overlapped --remix is not built")
        if args.segment is not None and not (0 < args.segment < float("inf")):
            p.error(f"--segment {args.segment}: a positive number of seconds")
        if args.overlap is not None and not 0 <= args.overlap < 1:
            p.error(f"--overlap {args.overlap}: a fraction of a second in [0, 1)")
    if args.hop_slices is not None and args.stream is None:
        p.error("--hop-slices counts the blocks of a --stream step; it needs --stream")
    if args.stream is not None:
        if args.stream < 1:
            p.error(f"--stream {args.stream}: a positive number of samples per block")
        if args.hop_slices is not None and args.hop_slices < 1:
            p.error(f"--hop-slices {args.hop_slices}: at least one block per step")
        if args.remix:
            p.error("--stream returns the four stems block by block; gains are not built into the session (weight the stems instead of --remix)")
        if args.segment is not None or args.overlap is not None:
            p.error("--stream has no chunk joints to fade; --segment / --overlap are for whole tracks")
        for opt in ("softmask", "residual"):
            if getattr(args, opt):
                p.error(f"--{opt} is an option of the Wiener filter, which cannot stream; --stream is mix-phase")
        if args.long_bands:
            p.error("--stream cannot run on a --long-bands plan: Separator.stream refuses it")
        if not args.realtime and (args.niter is None or args.niter >= 1):
            p.error("--stream is mix-phase: the Wiener-EM of the offline model (--niter >= 1, its default) spans 5000-frame windows and "
                    "cannot stream; use --realtime or --niter 0")
    return args


def cli_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="xumx-sliCQ-V2 inference on MI355X (hip-rocm backend)")
    p.add_argument("--input-dir", type=str, default="/input")
    p.add_argument("--output-dir", type=str, default="/output")
    p.add_argument("--ext", type=str, default=".wav")
    p.add_argument("--model-path", type=str, default=None,
                   help="directory with xumx_slicq_v2.json/.pth; omit for seeded synthetic weights")
    p.add_argument("--realtime", action="store_true")
    p.add_argument("--warmup", type=int, default=0)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--serial", action="store_true", help="one track at a time, as the reference's loop (inference.py:118-146)")
    p.add_argument("--remix", action="append", default=None, metavar="NAME:SPEC",
                   help="write <NAME>.wav = sum of the stems with the gains of SPEC (target=gain,...; unnamed targets keep 1.0) "
                        "instead of the four stems, e.g. karaoke:vocals=0; up to four times")
    p.add_argument("--niter", type=int, default=None, metavar="N",
                   help="EM iterations of the Wiener post-filter of the offline model (default 1, the reference's; 0 = mix-phase); "
                        "not with --realtime, which has no EM")
    p.add_argument("--softmask", action="store_true",
                   help="start the Wiener post-filter from the ratio mask instead of the mixture phase (norbert's use_softmask); "
                        "not with --realtime")
    p.add_argument("--residual", action="store_true",
                   help="add a fifth source holding what the four target models do not explain and write it as residual.wav beside "
                        "the four stems; not with --realtime or --remix")
    p.add_argument("--segment", type=float, default=None, metavar="SECONDS",
                   help="demix in overlapped, cross-faded segments of this hop (Separator.forward_overlapped, default 10.0 once "
                        "--segment or --overlap is given) instead of hard-joined chunks; not with --remix")
    p.add_argument("--overlap", type=float, default=None, metavar="FRACTION",
                   help="overlap of consecutive segments as a fraction of a second, in [0, 1) (default 0.1 once --segment or "
                        "--overlap is given); not with --remix")
    p.add_argument("--stream", type=int, default=None, metavar="BLOCK_SAMPLES",
                   help="push each file through a streaming session (Separator.stream) in blocks of this many samples and write the "
                        "four stems it returns; one track at a time; --realtime or --niter 0 only, not with --remix, --segment, "
                        "--overlap, --softmask, --residual")
    p.add_argument("--hop-slices", type=int, default=None, metavar="M",
                   help="blocks of sllen / 2 samples per step of the --stream session (default 1)")
    p.add_argument("--long-bands", action="store_true",
                   help="accept a model trained on the cqlog or vqlog scale: its bands above 320 samples run on the FFT band engine; "
                        "one track at a time, not with --stream")
    p.add_argument("--fgamma", type=float, default=15.0, metavar="HZ",
                   help="offset of the vqlog band centres where the model's JSON names none (default 15.0)")
    return p


def inference_main(argv=None):
    p = cli_parser()
    args = parse_args(p, argv)
    try:
        remix = parse_remix_specs(args.remix)
    except ValueError as e:
        p.error(str(e))
    if args.model_path:
        separator = Separator.load(model_path=args.model_path, runtime_backend="hip-rocm",
                                   warmup=args.warmup, realtime=args.realtime, device=args.device, niter=args.niter,
                                   softmask=args.softmask or None, residual=args.residual or None, long_bands=args.long_bands,
                                   fgamma=args.fgamma)
    else:
        separator = seeded_separator(realtime=args.realtime, device=args.device, niter=args.niter, softmask=args.softmask or None,
                                     residual=args.residual or None, long_bands=args.long_bands, fgamma=args.fgamma)
    if separator.long_bands:
        args.serial = True       # demix_directory batches tracks through demix_into, which such a plan does not serve
    overlapped = overlapped_option(args)
    if overlapped is not None:
        try:
            separator._segment_lengths(*overlapped)
        except ValueError as e:
            p.error(str(e))
    out_dir = Path(args.output_dir)
    wavs = sorted(Path(args.input_dir).glob(f"*{args.ext}"))
    if not args.serial and args.stream is None:
        t0 = time.time()
        done = demix_directory(separator, wavs, out_dir, device=args.device, remix=remix, overlapped=overlapped)
        wall = time.time() - t0
        if done:
            print(f"xumx-sliCQ-V2 inference time: {sum(d[2] for d in done) / len(done) / 1e3:.4f} s/track over {len(done)} track(s); "
                  f"{len(done) / wall:.2f} tracks/s end to end (decode, H2D, demix, D2H, encode)")
        return
    tot, n = 0.0, 0
    for wav in wavs:
        sig, rate = xaudio.load_audio(str(wav))
        if args.stream is not None:
            estimates, dt = _stream_one(sig, separator, rate, args.device, args.stream, args.hop_slices or 1)
        elif overlapped is not None:
            estimates, dt = _overlapped_one(sig, separator, rate, args.device, overlapped)
        elif remix is None:
            estimates, dt = separate(sig, separator, rate=rate, device=args.device)
        else:
            estimates, dt = _remix_one(sig, separator, rate, args.device, remix)
        tot, n = tot + dt, n + 1
        target_dir = out_dir / wav.stem
        target_dir.mkdir(parents=True, exist_ok=True)
        for target, est in estimates.items():
            xaudio.save_wav_float(str(target_dir / f"{target}.wav"), est[0], int(float(separator.sample_rate)))
        print(f"{wav.name}: {sig.shape[-1] / rate:.1f} s demixed in {dt * 1e3:.1f} ms")
    if n:
        print(f"xumx-sliCQ-V2 inference time: {tot / n:.4f} s/track over {n} track(s)")


if __name__ == "__main__":
    inference_main()
