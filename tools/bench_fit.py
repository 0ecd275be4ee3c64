"""What feeding the training step costs (BASELINE configs[4] shape: B = 16 excerpts of 88,200 samples, offline model):
  (a) Trainer.step on one fixed resident batch;
  (b) DeviceDataset.batch (one xsq_batch_assemble launch) + step;
  (c) the same batch built from torch ops (slice, multiply, flip, stack, sum: the path the kernel replaces) + step;
  (d) xsq_batch_assemble alone, both storages, next to a device-to-device copy that moves the same number of bytes
      (half of them read, half written), timed in the same run;
  (e) steps per second of one Trainer.fit epoch (training pass + validation + checkpoint) and of its training pass.
The arms are interleaved round by round; every figure is the median over the rounds with the min and max beside it.
Prints one JSON line per arm and appends them to --out.  Seeded synthetic pool: ten tracks of 20 - 40 s."""
import argparse, json, os, sys, tempfile, time
from contextlib import redirect_stdout
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from xumx_slicq_amd.data import DeviceDataset
from xumx_slicq_amd.separator import seeded_separator
from xumx_slicq_amd.training import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--seq-dur", type=float, default=2.0)
ap.add_argument("--tracks", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20, help="steps per arm and round")
ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16x6"])
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fit_bench.jsonl"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_fit.py measures on the GPU only"
B, n = a.batch, int(a.seq_dur * 44100)

rng = np.random.default_rng(20260101)
lengths = [int(v) for v in rng.integers(20 * 44100, 40 * 44100 + 1, size=a.tracks)]
tracks = [{s: rng.integers(-8000, 8000, size=(2, ln), dtype=np.int16) for s in DeviceDataset.sources} for ln in lengths]
pools = {st: DeviceDataset.from_arrays(tracks, storage=st) for st in ("pcm16", "fp32")}
train = pools["pcm16"]
valid = DeviceDataset.from_arrays([{s: v[:, :3 * 44100] for s, v in tracks[0].items()}], storage="pcm16")
del tracks
with redirect_stdout(sys.stderr):
    sep = seeded_separator(realtime=False)
tr = Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), precision=a.precision)
spt = max(1, -(-(a.steps + 1) * B // a.tracks))
table = train.draw_epoch(42, 1, B, a.seq_dur, samples_per_track=spt)
table32 = pools["fp32"].table(table.records, B, n)
steps = min(a.steps, table.nsteps - 1)                       # full batches only
fixed = tuple(t.clone() for t in train.batch(table, 0))


def torch_batch(ds, rec):
    """One batch from torch ops on the fp32 pool: per item and source a slice, a gain, a flip; a stack; a sum."""
    items = []
    for b in range(rec.shape[0]):
        cols = [None] * 4
        for s in range(4):
            t, start, swap = int(rec[b, s, 0]), int(rec[b, s, 1]), int(rec[b, s, 3])
            gain = float(rec[b, s, 2:3].view(np.float32)[0])
            off, st = int(ds.offsets[t]), (int(ds.lengths[t]) + 7) // 8 * 8
            v = ds.pool[off + 2 * s * st:off + (2 * s + 2) * st].view(2, st)[:, start:start + n] * gain
            cols[ds.target_of_column[s]] = v.flip(0) if swap else v
        items.append(torch.stack(cols))
    y = torch.stack(items, dim=1)
    return y.sum(0), y


def run_steps(make):
    pend = []
    for k in range(steps):
        pend.append(tr.step(*make(k), wait=False))
        if len(pend) == 3:
            pend.pop(0).result()
    for p in pend:
        p.result()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def assemble_only(ds, tab):
    for k in range(steps):
        ds.batch(tab, k)


nbytes = {st: B * 4 * 2 * n * (2 if st == "pcm16" else 4) + 5 * B * 2 * n * 4 for st in pools}
copies = {st: (torch.empty(nb // 2, dtype=torch.uint8, device="cuda"), torch.empty(nb // 2, dtype=torch.uint8, device="cuda"))
          for st, nb in nbytes.items()}


def copy_only(st):
    src, dst = copies[st]
    for _ in range(steps):
        dst.copy_(src)


arms = {
    "a_step_fixed_batch": lambda: run_steps(lambda k: fixed),
    "b_assemble_and_step": lambda: run_steps(lambda k: train.batch(table, k)),
    "c_torch_ops_and_step": lambda: run_steps(lambda k: torch_batch(pools["fp32"], table.records[k * B:(k + 1) * B])),
    "d_assemble_pcm16": lambda: assemble_only(pools["pcm16"], table),
    "d_copy_pcm16_bytes": lambda: copy_only("pcm16"),
    "d_assemble_fp32": lambda: assemble_only(pools["fp32"], table32),
    "d_copy_fp32_bytes": lambda: copy_only("fp32"),
}
# the torch path builds the same batch (to fp32 rounding of its sum order) -- checked once, outside the timed window
xk, yk = train.batch(table, 1)
xt, yt = torch_batch(pools["fp32"], table.records[B:2 * B])
assert torch.equal(yk, yt) and float((xk - xt).abs().max()) < 1e-5
for fn in arms.values():                                       # warm every shape the timed window uses
    fn()
ms = {name: [] for name in arms}
for _ in range(a.rounds):
    for name, fn in arms.items():
        ms[name].append(timed(fn) / steps)


def stat(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}


base = {"bench": "fit", "batch": B, "n": n, "tracks": a.tracks, "pool_seconds": round(sum(lengths) / 44100, 1), "precision": a.precision,
        "rounds": a.rounds, "steps_per_round": steps, "device": torch.cuda.get_device_name(0)}
lines = [dict(base, arm=name, **stat(v)) for name, v in ms.items()]
med = {name: float(np.median(v)) for name, v in ms.items()}
for st in pools:
    lines.append(dict(base, arm=f"d_{st}_summary", bytes=nbytes[st], assemble_gb_s=round(nbytes[st] / med[f"d_assemble_{st}"] / 1e6, 1),
                      copy_gb_s=round(nbytes[st] / med[f"d_copy_{st}_bytes"] / 1e6, 1),
                      assemble_over_copy=round(med[f"d_assemble_{st}"] / med[f"d_copy_{st}_bytes"], 3)))
lines.append(dict(base, arm="summary", b_minus_a_ms=round(med["b_assemble_and_step"] - med["a_step_fixed_batch"], 4),
                  c_minus_a_ms=round(med["c_torch_ops_and_step"] - med["a_step_fixed_batch"], 4),
                  a_spread_ms=round(float(np.max(ms["a_step_fixed_batch"]) - np.min(ms["a_step_fixed_batch"])), 4)))
# (e) one epoch of fit: 40 samples per track -> 25 steps of B = 16, validation over one 3 s track, checkpoint files
with tempfile.TemporaryDirectory() as d:
    epoch_table = train.draw_epoch(42, 2, B, a.seq_dur, samples_per_track=40)
    tr.train_epoch(train, epoch_table)
    t_pass = timed(lambda: tr.train_epoch(train, epoch_table))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.fit(train, valid, 1, batch_size=B, seq_dur=a.seq_dur, samples_per_track=40, model_path=d)
    t_fit = (time.perf_counter() - t0) * 1e3
    # where the rest of the epoch goes: the validation pass (weight hand-back + one piece) and the checkpoint's state + files
    t_valid = timed(lambda: tr.validate(valid))
    t_state = timed(tr.checkpoint_state)
    state = tr.checkpoint_state()
    t_save = timed(lambda: (torch.save({"state_dict": state[0], "optimizer": state[1]}, os.path.join(d, "c")), torch.save(state[0], os.path.join(d, "w"))))
lines.append(dict(base, arm="e_fit_epoch", steps=len(epoch_table), train_pass_steps_per_s=round(len(epoch_table) / t_pass * 1e3, 1),
                  train_pass_ms_per_step=round(t_pass / len(epoch_table), 4), fit_epoch_ms=round(t_fit, 1),
                  fit_epoch_steps_per_s=round(len(epoch_table) / t_fit * 1e3, 1), validate_ms=round(t_valid, 1),
                  checkpoint_state_ms=round(t_state, 1), checkpoint_save_ms=round(t_save, 1)))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a") as f:
    for line in lines:
        print(json.dumps(line))
        f.write(json.dumps(line) + "\n")
