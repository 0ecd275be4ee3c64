"""The epoch loop of ``xumx_slicq_amd.training.fit`` (training_main, training.py:478-556) against a fake trainer with
scripted losses: plateau schedule, early stopping, the reference's checkpoint files and resuming.  No GPU."""
import json
import math
import os

import pytest
import torch

from xumx_slicq_amd import training as T


class FakeData:
    def __init__(self):
        self.draws = []

    def draw_epoch(self, seed, epoch, batch_size, seq_dur, samples_per_track=64, augment=True):
        self.draws.append((seed, epoch, batch_size, seq_dur, samples_per_track))
        return ("table", epoch)


class FakeTrainer:
    """The part of ``Trainer`` that ``fit`` drives; validation losses come from a script indexed by epoch."""

    def __init__(self, valid_losses, lr=1e-3):
        self.script, self.lr, self.epochs_run, self.lrs = list(valid_losses), lr, [], []
        self.weights = torch.zeros(3)

    def train_epoch(self, train, table):
        assert table[0] == "table"
        self.epochs_run.append(table[1])
        self.lrs.append(self.lr)
        self.weights = self.weights + 1
        return 10.0 + table[1]

    def validate(self, valid, valid_chunk):
        return self.script[self.epochs_run[-1] - 1]

    def checkpoint_state(self):
        return {"w": self.weights.clone()}, {"state": {}, "param_groups": [{"lr": self.lr}]}

    def load_checkpoint(self, state_dict, optimizer):
        self.weights = state_dict["w"].clone()
        self.lr = optimizer["param_groups"][0]["lr"]

    def model_args(self):
        return {"fscale": "bark", "fbins": 262, "fmin": 32.9, "sample_rate": 44100.0, "nb_channels": 2, "realtime": False}


def _fit(tr, epochs, **kw):
    return T.fit(tr, FakeData(), FakeData(), epochs, **kw)


def test_plateau_schedule_lowers_the_lr_after_patience_bad_epochs_and_respects_the_cooldown():
    """ReduceLROnPlateau(factor=0.3, patience=2, cooldown=10): a best epoch, then bad ones.  The third bad epoch is the
    first past the patience: lr x 0.3 from the next epoch on; ten cooldown epochs count no bad epoch, so the next cut
    comes after cooldown + patience + 1 further bad epochs."""
    tr = FakeTrainer([1.0] + [2.0] * 40)
    hist = _fit(tr, 30, lr_decay_patience=2, lr_decay_gamma=0.3)
    assert hist["epochs_trained"] == 30 and tr.epochs_run == list(range(1, 31))
    cuts = [i + 1 for i in range(1, 30) if tr.lrs[i] != tr.lrs[i - 1]]      # epochs that train at a new lr
    assert cuts == [5, 18], cuts                                            # after epochs 4 and 4 + 10 + 3
    assert tr.lrs[3] == 1e-3 and tr.lrs[4] == pytest.approx(3e-4) and tr.lrs[17] == pytest.approx(9e-5)
    # the same numbers from torch's own scheduler on a real optimizer
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.3, patience=2, cooldown=10)
    want = []
    for loss in tr.script[:30]:
        want.append(opt.param_groups[0]["lr"])
        sch.step(loss)
    assert tr.lrs == want


def test_early_stopping_after_patience_bad_epochs_and_on_nan():
    tr = FakeTrainer([3.0, 2.0, 2.5, 2.5, 2.5, 2.5, 1.0])
    hist = _fit(tr, 20, patience=3)
    assert tr.epochs_run == [1, 2, 3, 4, 5] and hist["epochs_trained"] == 5
    assert (hist["best_loss"], hist["best_epoch"], hist["num_bad_epochs"]) == (2.0, 2, 3)
    assert hist["valid_loss_history"] == [3.0, 2.0, 2.5, 2.5, 2.5] and hist["train_loss_history"] == [11.0, 12.0, 13.0, 14.0, 15.0]
    tr = FakeTrainer([3.0, float("nan"), 1.0])
    hist = _fit(tr, 20, patience=1000)
    assert tr.epochs_run == [1, 2] and math.isnan(hist["valid_loss_history"][1]) and hist["best_loss"] == 3.0
    es = T._EarlyStopping(patience=2)                                       # training.py:590-622, step by step
    assert [es.step(v) for v in (5.0, 4.0, 4.0, 4.5)] == [False, False, False, True] and es.best == 4.0
    assert T._EarlyStopping(patience=2).step(float("nan")) is False        # the first value only sets `best` (training.py:606-608)


def test_checkpoint_files_hold_the_reference_keys_and_names(tmp_path):
    tr = FakeTrainer([3.0, 2.0, 2.5])
    data = FakeData()
    hist = T.fit(tr, data, FakeData(), 3, batch_size=4, seq_dur=1.0, samples_per_track=2, seed=7, model_path=str(tmp_path / "m"))
    assert data.draws == [(7, e, 4, 1.0, 2) for e in (1, 2, 3)]
    assert sorted(os.listdir(tmp_path / "m")) == ["xumx_slicq_v2.chkpnt", "xumx_slicq_v2.json", "xumx_slicq_v2.pth"]
    ck = torch.load(tmp_path / "m" / "xumx_slicq_v2.chkpnt", weights_only=False)
    assert sorted(ck) == ["best_loss", "epoch", "optimizer", "scheduler", "state_dict"]
    assert ck["epoch"] == 4 and ck["best_loss"] == 2.0 and torch.equal(ck["state_dict"]["w"], torch.full((3,), 3.0))
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]), factor=0.3,
                                                     patience=80, cooldown=10)
    assert sorted(ck["scheduler"]) == sorted(sch.state_dict())
    sch.load_state_dict(ck["scheduler"])
    assert sch.best == 2.0 and sch.num_bad_epochs == 1
    best = torch.load(tmp_path / "m" / "xumx_slicq_v2.pth")
    assert torch.equal(best["w"], torch.full((3,), 2.0))                     # written on the best epoch (2) only
    res = json.load(open(tmp_path / "m" / "xumx_slicq_v2.json"))
    for key in ("epochs_trained", "args", "best_loss", "best_epoch", "train_loss_history", "valid_loss_history",
                "train_time_history", "num_bad_epochs"):
        assert key in res, key
    assert {k: res[k] for k in hist} == hist
    for key in ("fscale", "fbins", "fmin", "sample_rate", "seq_dur", "realtime"):      # what load_target_models reads
        assert key in res["args"], key
    assert res["args"]["seq_dur"] == 1.0 and res["args"]["nb_channels"] == 2


def test_history_and_state_are_restored_on_resume(tmp_path):
    script = [3.0, 2.0, 2.5, 2.6, 1.5, 1.6]
    straight = FakeTrainer(script)
    want = _fit(straight, 6, lr_decay_patience=1, lr_decay_gamma=0.5, patience=4)
    first = FakeTrainer(script)
    _fit(first, 3, lr_decay_patience=1, lr_decay_gamma=0.5, patience=4, model_path=str(tmp_path))
    resumed = FakeTrainer(script, lr=123.0)                                   # everything comes from the checkpoint
    got = _fit(resumed, 6, lr_decay_patience=1, lr_decay_gamma=0.5, patience=4, model_path=str(tmp_path))
    assert resumed.epochs_run == [4, 5, 6] and first.lrs + resumed.lrs == straight.lrs
    assert straight.lrs[3] == 1e-3 and straight.lrs[4] == 5e-4               # the cut falls in the resumed half
    for key in ("epochs_trained", "best_loss", "best_epoch", "train_loss_history", "valid_loss_history", "num_bad_epochs"):
        assert got[key] == want[key], key
    assert len(got["train_time_history"]) == 6 and torch.equal(resumed.weights, straight.weights)
    # a finished run resumes to nothing
    again = FakeTrainer(script)
    assert _fit(again, 6, model_path=str(tmp_path))["epochs_trained"] == 6 and again.epochs_run == []
