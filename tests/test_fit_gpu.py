"""``Trainer.fit`` on the device against the loop written out by hand (``draw_epoch``, ``batch``, ``Trainer.step``,
``loss.validation_step``): seeded Bark-262 offline model as in tests/test_training.py, B = 2 one-second excerpts, three
synthetic training tracks of 1.5 - 3 s (two excerpts per track: three steps per epoch), one validation track cut into
pieces of 30,000 samples, the last of which (6,150 samples) is below the model's minimum length and gets zero-padded.

The rule of comparison: two runs of the hand loop on the same batches are compared first.  MEASURED on MI355X: they agree
BITWISE (losses, validation losses and every tensor of the final state_dict), so ``fit`` -- and a run resumed from a
checkpoint -- must equal the hand loop bitwise.  Should two hand-loop runs ever differ, ``close`` below holds ``fit`` to the
spread they show instead: its distance to the nearer run no larger than the distance between the two."""
import json
import os

import numpy as np
import pytest
import torch

from xumx_slicq_amd.synth import synth_audio

pytestmark = pytest.mark.gpu

SEED, B, SEQ, SPT, CHUNK, EPOCHS = 42, 2, 1.0, 2, 30000, 2
KW = dict(batch_size=B, seq_dur=SEQ, samples_per_track=SPT, seed=SEED, valid_chunk=CHUNK)


def _datasets():
    from xumx_slicq_amd.data import DeviceDataset
    def track(n, seed, pcm):
        stems = {s: 0.4 * synth_audio(n, seed=seed + j)[0].numpy() for j, s in enumerate(DeviceDataset.sources)}
        return {s: np.rint(v * 32768).astype(np.int16) for s, v in stems.items()} if pcm else stems
    train = DeviceDataset.from_arrays([track(n, 900 + 10 * i, True) for i, n in enumerate((66150, 97021, 132300))], storage="pcm16")
    valid = DeviceDataset.from_arrays([track(66150, 950, False)], storage="fp32")
    return train, valid


def _trainer():
    from xumx_slicq_amd.separator import seeded_separator
    from xumx_slicq_amd.training import Trainer
    sep = seeded_separator(realtime=False)
    return sep, Trainer(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm))


def hand_loop(train, valid, epochs):
    from xumx_slicq_amd.loss import validation_step
    sep, tr = _trainer()
    floor = 18060 // 2 + 1
    train_losses, valid_losses = [], []
    for epoch in range(1, epochs + 1):
        table = train.draw_epoch(SEED, epoch, B, SEQ, SPT)
        assert len(table) == 3
        train_losses.append(float(np.mean([tr.step(*train.batch(table, k))[0] for k in range(len(table))])))
        tr.sync_to(sep.xumx_model)
        vl = []
        for x, y in valid.pieces(0, CHUNK):
            if x.shape[-1] < floor:
                x = torch.nn.functional.pad(x, (0, floor - x.shape[-1]))
                y = torch.nn.functional.pad(y, (0, floor - y.shape[-1]))
            vl.append(validation_step(sep.xumx_model, (sep.nsgt, sep.insgt, sep.cnorm), x, y)[0])
        assert len(vl) == 3
        valid_losses.append(float(np.mean(vl)))
    return {"train": train_losses, "valid": valid_losses, "state": tr.state_dict()}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    train, valid = _datasets()
    a, b = hand_loop(train, valid, EPOCHS), hand_loop(train, valid, EPOCHS)
    path = str(tmp_path_factory.mktemp("fit") / "model")
    sep, tr = _trainer()
    hist = tr.fit(train, valid, EPOCHS, model_path=path, **KW)
    f = {"train": hist["train_loss_history"], "valid": hist["valid_loss_history"], "state": tr.state_dict()}
    bitwise = a["train"] == b["train"] and a["valid"] == b["valid"] and all(torch.equal(a["state"][k], b["state"][k]) for k in a["state"])
    print(f"\n[fit] two hand loops bitwise equal: {bitwise}; train {a['train']} / {b['train']}, valid {a['valid']} / {b['valid']}; "
          f"fit train {f['train']}, valid {f['valid']}")
    return {"train": train, "valid": valid, "a": a, "b": b, "fit": f, "hist": hist, "path": path, "bitwise": bitwise}


def close(got, a, b, bitwise):
    """``got`` against the two hand-loop runs ``a`` and ``b``: bitwise when they agree bitwise, else within their spread."""
    for key in ("train", "valid"):
        for g, u, v in zip(got[key], a[key], b[key]):
            print(f"[fit] {key}: {g!r} against {u!r} / {v!r}")
            assert g == u if bitwise else min(abs(g - u), abs(g - v)) <= abs(u - v), (key, g, u, v)
    assert len(got["train"]) == len(a["train"]) and len(got["valid"]) == len(a["valid"])
    for k in a["state"]:
        if bitwise:
            assert torch.equal(got["state"][k], a["state"][k]), k
        else:
            spread = float((a["state"][k] - b["state"][k]).abs().max())
            d = min(float((got["state"][k] - a["state"][k]).abs().max()), float((got["state"][k] - b["state"][k]).abs().max()))
            assert d <= spread, (k, d, spread)


def test_fit_equals_the_hand_loop(runs):
    assert runs["bitwise"]                     # the measured premise of this file's docstring
    close(runs["fit"], runs["a"], runs["b"], runs["bitwise"])
    h = runs["hist"]
    assert h["epochs_trained"] == EPOCHS and len(h["train_time_history"]) == EPOCHS
    assert h["best_loss"] == min(h["valid_loss_history"]) and h["best_epoch"] == 1 + int(np.argmin(h["valid_loss_history"]))
    assert all(np.isfinite(h["train_loss_history"])) and all(np.isfinite(h["valid_loss_history"]))


def test_a_resumed_run_equals_two_epochs_straight(runs, tmp_path):
    path = str(tmp_path / "model")
    _, first = _trainer()
    h1 = first.fit(runs["train"], runs["valid"], 1, model_path=path, **KW)
    assert h1["epochs_trained"] == 1
    _, second = _trainer()                                       # a fresh trainer: everything comes from the checkpoint
    h2 = second.fit(runs["train"], runs["valid"], EPOCHS, model_path=path, **KW)
    got = {"train": h2["train_loss_history"], "valid": h2["valid_loss_history"], "state": second.state_dict()}
    close(got, runs["a"], runs["b"], runs["bitwise"])
    assert h2["epochs_trained"] == EPOCHS and second.steps == 6
    for key in ("best_loss", "best_epoch", "num_bad_epochs"):
        assert h2[key] == runs["hist"][key], key
    straight = torch.load(os.path.join(runs["path"], "xumx_slicq_v2.chkpnt"), weights_only=False)
    resumed = torch.load(os.path.join(path, "xumx_slicq_v2.chkpnt"), weights_only=False)
    assert straight["epoch"] == resumed["epoch"] == EPOCHS + 1 and straight["scheduler"] == resumed["scheduler"]
    if runs["bitwise"]:
        k = "sliced_umx.1.cdaes.0.4.num_batches_tracked"
        assert int(straight["state_dict"][k]) == int(resumed["state_dict"][k])
        i = len(straight["optimizer"]["state"]) - 1
        assert torch.equal(straight["optimizer"]["state"][i]["exp_avg_sq"], resumed["optimizer"]["state"][i]["exp_avg_sq"])
        assert float(resumed["optimizer"]["state"][i]["step"]) == 6.0


def test_saved_model_loads_through_separator_load_and_demixes(runs):
    from xumx_slicq_amd.separator import Separator
    path = runs["path"]
    assert sorted(os.listdir(path)) == ["xumx_slicq_v2.chkpnt", "xumx_slicq_v2.json", "xumx_slicq_v2.pth"]
    args = json.load(open(os.path.join(path, "xumx_slicq_v2.json")))["args"]
    assert (args["fscale"], args["fbins"], args["fmin"], args["sample_rate"], args["seq_dur"], args["realtime"]) == \
        ("bark", 262, 32.9, 44100.0, SEQ, False)
    sep = Separator.load(model_path=path)
    saved = torch.load(os.path.join(path, "xumx_slicq_v2.pth"))
    loaded = sep.xumx_model.state_dict()
    assert sorted(saved) == sorted(loaded) and all(torch.equal(saved[k].cpu(), loaded[k].cpu()) for k in saved)
    if runs["hist"]["best_epoch"] == EPOCHS:                      # the last epoch was the best: the file holds the final weights
        assert all(torch.equal(saved[k].cpu(), v) for k, v in runs["fit"]["state"].items())
    est = sep(synth_audio(9031, seed=77).cuda())
    assert est.shape == (4, 1, 2, 9031) and bool(torch.isfinite(est).all()) and float(est.abs().max()) > 0
