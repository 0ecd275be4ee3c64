"""Mirror of the training half of /root/reference/xumx_slicq_v2/training.py:34-112 (``loop`` with
``train=True``) on the HIP library: one call = forward with BatchNorm on batch statistics, ComplexMSE +
MaskSum loss (+ ``sdr_mcoef`` x the SDR criterion on the estimates' waveforms when ``sdr_mcoef > 0``, training.py:94-103),
backward of every trainable tensor, AdamW update (training.py:391-393 defaults).

The reference hands the step to torch autograd + ``torch.optim.AdamW``; here the whole step is
``xsq_train_step`` (csrc/train.hip) over flat parameter / gradient / moment pools that keep the
reference's state_dict order, so a checkpoint of the reference loads, trains and saves unchanged.
With the SDR term on the step is ``xsq_train_step_sdr``: the estimates' inverse sliCQT, the SD-SDR passes (csrc/sdr.hip) and
the adjoint of the inverse transform into the estimates' gradient run inside it; with the term off (the default,
``--sdr-mcoef -1``) the step is the one it was.

``Trainer.fit`` (``fit`` below) is the loop ``training_main`` has around the step (training.py:478-556): per epoch a
training pass over batches that ``data.DeviceDataset`` assembles on the device, a validation pass, the plateau LR
schedule, early stopping and the reference's checkpoint files; ``python -m xumx_slicq_amd.training`` is its command line.
The LSTM variant, ``PeripheryDataset``, tensorboard / torchinfo / tqdm output and data-parallel training are not mirrored."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import time
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .model import Unmix


class PendingLoss:
    """Loss of a step issued with ``wait=False``: ``result()`` (or indexing / iteration, like the tuple ``step``
    returns) blocks until THAT step has finished on the device.  Valid for the trainer's last four steps."""

    def __init__(self, trainer: "Trainer", ticket: int, sdr_mcoef: float = -1.0):
        self._trainer, self._ticket, self._value, self._sdr_mcoef = trainer, int(ticket), None, float(sdr_mcoef)

    def result(self) -> Tuple[float, ...]:
        if self._value is None and self._sdr_mcoef > 0:
            out = (C.c_double * 3)()
            _lib.call("xsq_train_loss_sdr", self._trainer._h, self._ticket, out)
            mse, mask, sdr = float(out[0]), float(out[1]), float(out[2])
            self._value = (mse + mask + self._sdr_mcoef * sdr, mse, mask, sdr)
        if self._value is None:
            out = (C.c_double * 2)()
            _lib.call("xsq_train_loss", self._trainer._h, self._ticket, out)
            mse, mask = float(out[0]), float(out[1])
            self._value = (mse + mask, mse, mask)
        return self._value

    def __getitem__(self, i):
        return self.result()[i]

    def __iter__(self):
        return iter(self.result())


class Trainer:
    """Owns the device-side training state of one ``Unmix``.

    ``step(x, y_targets)`` = the body of ``for x, y in pbar`` (training.py:66-110) and returns
    ``(loss, mse_loss, mask_loss)`` as python floats -- with ``sdr_mcoef > 0`` (training.py:94: the term is on)
    ``(loss, mse_loss, mask_loss, sdr_loss)``, ``sdr_loss`` the unweighted criterion and
    ``loss = mse_loss + mask_loss + sdr_mcoef * sdr_loss``; ``gradients()`` exposes what
    ``loss.backward()`` would have left in ``.grad``; ``state_dict()`` / ``sync_to(unmix)`` hand
    the trained tensors back in the reference's layout."""

    def __init__(self, unmix: Unmix, encoder, lr: float = 1e-3, weight_decay: float = 1e-5,
                 device: str | torch.device = "cuda", precision: str = "fp32", sdr_mcoef: float = -1.0):
        self.device = torch.device(device)
        self.sdr_mcoef = float(sdr_mcoef)
        if self.device.type != "cuda":
            raise _lib.XsqError("training runs on a ROCm device only; there is no CPU fallback")
        self.nsgt, self.insgt, self.cnorm = encoder
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.unmix = unmix                       # fit() hands the trained tensors back to it for validation and checkpoints
        self.table = unmix.table
        self._F, self._T = unmix._F, unmix._T
        causal = {blk.causal for blk in unmix.sliced_umx}
        wiener = {not blk.realtime for blk in unmix.sliced_umx}
        if len(causal) != 1 or len(wiener) != 1:
            raise _lib.XsqError("all blocks must share the same first-layer type and post-filter")
        self.causal, self.wiener = causal.pop(), wiener.pop()
        for opt in ("softmask", "residual"):
            if bool(getattr(unmix, opt, False)):
                raise _lib.XsqError(f"the training step differentiates the reference's filter (mix-phase start, four sources); this model "
                                    f"has {opt} = True: set it to False for training")
        if self.wiener and int(getattr(unmix, "niter", 1)) != 1:
            raise _lib.XsqError(f"training differentiates ONE Wiener-EM iteration (the reference trains with iterations=1, and the "
                                f"backward kernels are the gradient of one); this model has niter = {unmix.niter}: set it to 1 "
                                "to train and back afterwards")
        if getattr(getattr(getattr(self.nsgt, "nsgt", None), "plan", None), "dc_twins", False):
            raise _lib.XsqError("training on a plan with bands across DC (dc_twins = True) is not supported: the training step has not "
                                "been held to the reference on such a plan; build the plan without the flag (it is then refused by name)")
        if getattr(getattr(getattr(self.nsgt, "nsgt", None), "plan", None), "long_bands", False):
            raise _lib.XsqError("training on a plan with bands on the FFT band engine (long_bands = True) is not supported: the training "
                                "step's kernels have not been taken through blocks of thousands of frames")
        self._spec = [(k, tuple(v.shape)) for k, v in unmix.state_dict().items() if not k.endswith("num_batches_tracked")]
        params = unmix.packed_parameters()
        self.nparams = int(params.size)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.call("xsq_train_create", C.byref(self._h), len(self.table), self._F.ctypes.data, self._T.ctypes.data,
                      1 if self.causal else 0, params.ctypes.data, params.size)
        if precision not in ("fp32", "bf16x6", "bf16"):
            raise ValueError(f"precision {precision!r}: the training step offers 'fp32', 'bf16x6' and 'bf16'")
        self.precision = precision
        from .model import note_precision
        note_precision(self, precision)          # bf16x6: no packed-fp32 slice FFT in this process meanwhile
        # "bf16": the reference's autocast arithmetic for the convolutions (training.py:473-476): operands rounded to bf16, fp32 accumulate
        _lib.call("xsq_train_set_precision", self._h, {"fp32": 0, "bf16": 1, "bf16x6": 2}[precision])
        self._ws = None
        self._need = {}          # workspace bytes per step shape
        self._side = None        # stream of the targets' transform, made by the first step()
        self.steps = 0
        self._synced = 0         # steps already counted into num_batches_tracked by sync_to

    def __del__(self):
        try:
            from .model import note_precision
            note_precision(self, "fp32")
            if self._h:
                _lib.lib.xsq_train_destroy(self._h)
        except Exception:
            pass

    # -- one step ------------------------------------------------------------------------
    def _issue(self, key, workspace, launch, keep, nterms: int, apply_update: bool, wait: bool):
        """One step through either entry point: ``workspace()`` -> bytes (cached per ``key``), ``launch(out, ws)`` -> status with
        ``out`` the HOST double[nterms] the step waits for or None, ``keep`` the tensors its kernels read."""
        sdr = nterms == 3
        name = "xsq_train_step_sdr" if sdr else "xsq_train_step"
        with torch.cuda.device(self.device):
            need = self._need.get(key)
            if need is None:
                need = workspace()
                if need == 0:
                    raise _lib.XsqError(("xsq_train_workspace_sdr" if sdr else "xsq_train_workspace") + ": bad shape")
                self._need[key] = need
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            out = (C.c_double * nterms)() if wait else None
            _lib.check(launch(out, self._ws), name)
            if not wait:     # the arenas must outlive the kernels that read them: hand them to the pending object
                pending = PendingLoss(self, int(_lib.lib.xsq_train_ticket(self._h)), self.sdr_mcoef if sdr else -1.0)
                pending._keep = keep
        if apply_update:
            self.steps += 1
        if not wait:
            return pending
        mse, mask = float(out[0]), float(out[1])
        if not sdr:
            return mse + mask, mse, mask
        return mse + mask + self.sdr_mcoef * float(out[2]), mse, mask, float(out[2])

    def step_arena(self, X: Tensor, Yt: Tensor, B: int, S: int, apply_update: bool = True, wait: bool = True):
        """X: mix arena (2B channels), Yt: target arena (8B channels), both flat fp32 on the device.
        ``wait=False``: returns a ``PendingLoss`` without waiting for the device (the next step can be issued before
        this one's loss is looked at; the reference's ``loss.item()`` every step, training.py:110, is ``wait=True``)."""
        if self.sdr_mcoef > 0:
            raise _lib.XsqError("step_arena has no waveforms: the SDR term (sdr_mcoef > 0) needs step(x, y_targets)")
        w = 1 if self.wiener else 0
        return self._issue((B, S), lambda: _lib.lib.xsq_train_workspace(self._h, B, S, w),
                           lambda out, ws: _lib.lib.xsq_train_step(self._h, X.data_ptr(), Yt.data_ptr(), B, S, w, self.lr, self.weight_decay,
                                                                   1 if apply_update else 0, out, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                           (X, Yt), 2, apply_update, wait)

    @torch.no_grad()
    def step(self, x: Tensor, y_targets: Tensor, apply_update: bool = True, wait: bool = True):
        """x (B, 2, N) mix, y_targets (4, B, 2, N): training.py:66-108.  Returns (loss, mse, mask) -- or, with
        ``wait=False``, a ``PendingLoss`` that resolves to the same tuple."""
        x = x.to(self.device, torch.float32)
        y_targets = y_targets.to(self.device, torch.float32)
        # the two transforms are independent: the targets' (4x the rows) goes to a side stream beside the mix's
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side
        # (straight to the arenas: the module API's list of 70 block views per transform -- built, checked back into an arena
        #  and record_stream'ed one by one -- cost ~0.3 ms of host time per step during which the device sat idle,
        #  profiles/r07h_timeline_train.txt)
        eng = self.nsgt.nsgt.nsgt
        side.wait_stream(main)
        with torch.cuda.stream(side):
            Ytg, lead_t, S_t = eng.forward(y_targets)
        X, lead, S = eng.forward(x)
        main.wait_stream(side)
        Ytg.record_stream(main)
        if len(lead) != 2 or lead[1] != 2 or lead_t != (4, lead[0], 2) or S != S_t:
            raise ValueError(f"expected x (B, 2, N) and y_targets (4, B, 2, N); got arenas {lead} / {lead_t}")
        if self.sdr_mcoef > 0:
            return self._step_sdr(X, Ytg, y_targets.contiguous(), lead[0], S, apply_update, wait)
        return self.step_arena(X, Ytg, lead[0], S, apply_update, wait)

    def _step_sdr(self, X: Tensor, Yt: Tensor, y_targets: Tensor, B: int, S: int, apply_update: bool, wait: bool):
        """The step with the SDR term (xsq_train_step_sdr): the arenas of ``step`` plus the target waveforms."""
        n, w = int(y_targets.shape[-1]), 1 if self.wiener else 0
        plan = self.nsgt.nsgt.nsgt.handle(self.device)
        return self._issue((B, S, n), lambda: _lib.lib.xsq_train_workspace_sdr(self._h, plan, B, S, w, n),
                           lambda out, ws: _lib.lib.xsq_train_step_sdr(self._h, plan, X.data_ptr(), Yt.data_ptr(), y_targets.data_ptr(), n,
                                                                       self.sdr_mcoef, B, S, w, self.lr, self.weight_decay,
                                                                       1 if apply_update else 0, out, ws.data_ptr(), ws.numel(),
                                                                       _lib.stream_ptr()),
                           (X, Yt, y_targets), 3, apply_update, wait)

    # -- state ---------------------------------------------------------------------------
    def _read(self, what: int) -> "OrderedDict[str, Tensor]":
        buf = np.empty(self.nparams, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.call("xsq_train_read", self._h, what, buf.ctypes.data)
        out, o = OrderedDict(), 0
        for k, shp in self._spec:
            n = int(np.prod(shp)) if shp else 1
            out[k] = torch.from_numpy(buf[o:o + n].reshape(shp).copy())
            o += n
        return out

    def state_dict(self) -> "OrderedDict[str, Tensor]":
        """Parameters and BatchNorm running statistics, reference key layout (num_batches_tracked left out)."""
        return self._read(0)

    def gradients(self) -> Dict[str, Tensor]:
        """Gradients of the last step for every trainable tensor (the running statistics have none)."""
        return OrderedDict((k, v) for k, v in self._read(1).items()
                           if not k.endswith(("running_mean", "running_var")))

    def _write(self, what: int, tensors: Dict[str, Tensor]):
        buf = np.empty(self.nparams, dtype=np.float32)
        o = 0
        for k, shp in self._spec:
            n = int(np.prod(shp)) if shp else 1
            v = tensors[k]
            if tuple(v.shape) != tuple(shp):
                raise ValueError(f"{k}: shape {tuple(v.shape)} does not match {tuple(shp)}")
            buf[o:o + n] = v.detach().to("cpu", torch.float32).reshape(-1).numpy()
            o += n
        with torch.cuda.device(self.device):
            _lib.call("xsq_train_write", self._h, what, buf.ctypes.data)

    def _trainable(self):
        """Keys of ``unmix.parameters()`` in the order torch.optim.AdamW numbers them (training.py:391-393): the
        state_dict order without the BatchNorm running statistics (buffers)."""
        return [k for k, _ in self._spec if not k.endswith(("running_mean", "running_var"))]

    def optimizer_state_dict(self) -> dict:
        """``torch.optim.AdamW.state_dict()`` as the reference checkpoints it (training.py:419-430, :526): ``state``
        {parameter index: {step, exp_avg, exp_avg_sq}} over ``unmix.parameters()`` and ONE entry in ``param_groups``
        (lr, betas, eps, weight_decay, params) -- a reference ``.chkpnt``'s ``checkpoint["optimizer"]`` loads here and
        what is saved here loads into the reference's optimizer.  Before the first step ``state`` is empty, as torch's."""
        step = int(_lib.lib.xsq_train_step_count(self._h, -1))
        if step < 0:
            raise _lib.XsqError(f"xsq_train_step_count failed ({step}): {_lib.last_error()}")
        keys = self._trainable()
        state = {}
        if step > 0:
            m, v = self._read(2), self._read(3)
            state = {i: {"step": torch.tensor(float(step)), "exp_avg": m[k], "exp_avg_sq": v[k]} for i, k in enumerate(keys)}
        group = {"lr": self.lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(keys)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, state: dict):
        """Resume from ``optimizer.state_dict()`` (torch AdamW layout, see above): restores both moments and the step
        counter, so bias correction continues where it stopped.  One parameter group, one common step count (what a
        single AdamW over ``unmix.parameters()`` produces); anything else is rejected."""
        groups = state["param_groups"]
        keys = self._trainable()
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(keys))):
            raise ValueError(f"expected one param group over {len(keys)} parameters (torch.optim.AdamW(unmix.parameters()))")
        g = groups[0]
        if tuple(g.get("betas", (0.9, 0.999))) != (0.9, 0.999) or float(g.get("eps", 1e-8)) != 1e-8 or g.get("amsgrad", False):
            raise ValueError("the step implements AdamW with betas (0.9, 0.999), eps 1e-8, amsgrad off (training.py:391-393)")
        st = state["state"]
        shapes = dict(self._spec)
        if st:
            if sorted(st) != list(range(len(keys))):
                raise ValueError("optimizer state must cover every parameter (or none)")
            steps = {int(float(st[i]["step"])) for i in st}
            if len(steps) != 1:
                raise ValueError(f"parameters disagree on the step count: {sorted(steps)[:4]}")
            step = steps.pop()
        else:
            step = 0
        for what, name in ((2, "exp_avg"), (3, "exp_avg_sq")):
            full = {k: torch.zeros(shapes[k]) for k, _ in self._spec}          # running statistics carry no moments
            for i, k in enumerate(keys):
                if st:
                    full[k] = st[i][name]
            self._write(what, full)
        rc = int(_lib.lib.xsq_train_step_count(self._h, step))
        if rc < 0:
            raise _lib.XsqError(f"xsq_train_step_count failed ({rc}): {_lib.last_error()}")
        self.steps = step
        self._synced = self.steps
        self.lr = float(g.get("lr", self.lr))
        self.weight_decay = float(g.get("weight_decay", self.weight_decay))

    def load_state_dict(self, sd: Dict[str, Tensor]):
        """Parameters + running statistics from a (reference-layout) state_dict."""
        self._write(0, sd)

    def sync_to(self, unmix: Unmix) -> Unmix:
        """Hands the trained tensors to ``unmix``; ``num_batches_tracked`` advances by the steps taken SINCE
        THE LAST sync (calling this once per epoch must not count earlier epochs again)."""
        sd = unmix.state_dict()
        for k, v in self.state_dict().items():
            sd[k] = v
        fresh = self.steps - self._synced
        for k in sd:
            if k.endswith("num_batches_tracked"):
                sd[k] = sd[k] + fresh
        unmix.load_state_dict(sd, strict=True)
        self._synced = self.steps
        return unmix

    # -- the loop around the step (training.py:34-112, 478-556) -------------------------------------
    def train_epoch(self, train, table) -> float:
        """One training pass (training.py:34-112, train=True) over the batches of ``table``: every step is issued with
        ``wait=False``, at most three are in flight, and losses are read as they resolve.  Returns the plain mean of the
        batch losses (the reference's ``_AverageMeter`` weights every batch by ``x.size(1)``, a constant)."""
        pending, losses = [], []
        for k in range(len(table)):
            x, y = train.batch(table, k)
            pending.append(self.step(x, y, wait=False))
            if len(pending) == 3:
                losses.append(pending.pop(0)[0])
        losses.extend(p[0] for p in pending)
        return float(np.mean(losses))

    def validate(self, valid, valid_chunk: int = 2621440) -> float:
        """One validation pass (training.py:34-112, train=False): the unmix takes the current weights (``sync_to``) and
        ``loss.validation_step`` runs over ``valid.pieces(i, valid_chunk)`` of every track; the mean over pieces.
        A piece below the model's minimum length (half a slice + 1, separator.py:162) is zero-padded to it."""
        from .loss import validation_step
        unmix = self.sync_to(self.unmix).eval()
        encoder = (self.nsgt, self.insgt, self.cnorm)
        floor = self.nsgt.nsgt.plan.L // 2 + 1
        losses = []
        for i in range(len(valid)):
            for x, y in valid.pieces(i, valid_chunk):
                if x.shape[-1] < floor:
                    pad = floor - x.shape[-1]
                    x, y = torch.nn.functional.pad(x, (0, pad)), torch.nn.functional.pad(y, (0, pad))
                losses.append(validation_step(unmix, encoder, x, y, sdr_mcoef=self.sdr_mcoef)[0])
        return float(np.mean(losses))

    def checkpoint_state(self) -> Tuple[dict, dict]:
        """(``unmix.state_dict()`` with the current weights, ``optimizer.state_dict()``): training.py:524-526.  The tensors
        go into a plain OrderedDict: the module's own carries a ``_metadata`` attribute whose "version" entry of the root is
        the bound method ``Unmix._version`` -- pickling it would drag the whole module into the file, and
        ``torch.load(weights_only=True)`` (load_target_models) refuses it."""
        return OrderedDict(self.sync_to(self.unmix).state_dict()), self.optimizer_state_dict()

    def load_checkpoint(self, state_dict: dict, optimizer: dict):
        """training.py:419-420 (the reference loads with strict=False; every trained tensor must be there here)."""
        self.load_state_dict({k: state_dict[k] for k, _ in self._spec})
        self.load_optimizer_state_dict(optimizer)
        self.unmix.load_state_dict(state_dict, strict=False)
        self._synced = self.steps

    def model_args(self) -> dict:
        """The ``args`` of xumx_slicq_v2.json that ``separator.load_target_models`` reads (training.py:536)."""
        plan = self.nsgt.nsgt.plan
        return {"fscale": plan.scale, "fbins": int(plan.fbins), "fmin": float(plan.fmin), "sample_rate": float(plan.fs),
                "nb_channels": 2, "realtime": not self.wiener, "lr": self.lr, "weight_decay": self.weight_decay,
                "sdr_mcoef": self.sdr_mcoef, "precision": self.precision}

    def fit(self, train, valid, epochs: int, **kwargs) -> dict:
        """``fit(self, train, valid, epochs, ...)`` below."""
        return fit(self, train, valid, epochs, **kwargs)


class _EarlyStopping:
    """training.py:590-630 (mode "min", min_delta 0): ``step`` returns True when training should stop -- after
    ``patience`` epochs without a new best, and at once on a NaN loss."""

    def __init__(self, patience: int = 10):
        self.patience, self.best, self.num_bad_epochs = patience, None, 0

    def step(self, metrics) -> bool:
        if self.best is None:
            self.best = metrics
            return False
        if math.isnan(metrics):
            return True
        if self.patience == 0 or metrics < self.best:
            self.num_bad_epochs = 0
            self.best = metrics
        else:
            self.num_bad_epochs += 1
        return self.num_bad_epochs >= self.patience


CHECKPOINT, WEIGHTS, RESULTS = "xumx_slicq_v2.chkpnt", "xumx_slicq_v2.pth", "xumx_slicq_v2.json"


def fit(trainer, train, valid, epochs: int, batch_size: int = 32, seq_dur: float = 2.0, samples_per_track: int = 64,
        seed: int = 42, patience: int = 1000, lr_decay_patience: int = 80, lr_decay_gamma: float = 0.3,
        model_path: Optional[str] = None, valid_chunk: int = 2621440, quiet: bool = True) -> dict:
    """The epoch loop of ``training_main`` (training.py:478-556) around ``trainer`` (a ``Trainer``): epochs 1 .. ``epochs``,
    each ``train.draw_epoch(seed, epoch, ...)`` + ``trainer.train_epoch`` and ``trainer.validate(valid, valid_chunk)``;
    ``torch.optim.lr_scheduler.ReduceLROnPlateau(factor=lr_decay_gamma, patience=lr_decay_patience, cooldown=10)`` on
    the validation loss (training.py:401-406) -- it steps a one-parameter shim optimizer that carries ``trainer.lr``, so
    its ``state_dict()`` is the reference's, and the shim's lr is copied back to ``trainer.lr`` after every step --;
    ``_EarlyStopping(patience)``; and, with ``model_path``, per epoch the reference's files (training.py:521-546, 563-568):
    ``xumx_slicq_v2.chkpnt`` {epoch, state_dict, best_loss, optimizer, scheduler}, ``xumx_slicq_v2.pth`` (the weights) on
    a best epoch, ``xumx_slicq_v2.json`` (histories + the ``args`` ``load_target_models`` reads).  A ``model_path`` that
    already holds a checkpoint is resumed (training.py:411-435).  Returns the history dict the json holds.

    Departures from the reference: validation runs over pieces of ``valid_chunk`` samples (the Separator's chunk size)
    instead of whole tracks, so that no kernel's 32-bit range depends on a track's length; a resumed run continues with
    epoch ``epochs_trained + 1`` (the reference's ``trange`` starts at ``epochs_trained`` and repeats that epoch number);
    an epoch's time is in the json that epoch writes (the reference appends it after writing); no tensorboard, torchinfo
    or tqdm: ``quiet=False`` prints one line per epoch."""
    shim = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=trainer.lr)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(shim, factor=lr_decay_gamma, patience=lr_decay_patience, cooldown=10)
    es = _EarlyStopping(patience=patience)
    hist = {"epochs_trained": 0, "best_loss": None, "best_epoch": 0, "train_loss_history": [], "valid_loss_history": [],
            "train_time_history": [], "num_bad_epochs": 0}
    if model_path is not None:
        os.makedirs(model_path, exist_ok=True)
        if os.path.exists(os.path.join(model_path, CHECKPOINT)):
            with open(os.path.join(model_path, RESULTS), "r") as stream:
                hist = {k: v for k, v in json.load(stream).items() if k in hist}
            checkpoint = torch.load(os.path.join(model_path, CHECKPOINT), map_location="cpu", weights_only=False)
            trainer.load_checkpoint(checkpoint["state_dict"], checkpoint["optimizer"])
            scheduler.load_state_dict(checkpoint["scheduler"])
            shim.param_groups[0]["lr"] = trainer.lr
            es.best, es.num_bad_epochs = hist["best_loss"], hist["num_bad_epochs"]
    for epoch in range(hist["epochs_trained"] + 1, epochs + 1):
        end = time.time()
        table = train.draw_epoch(seed, epoch, batch_size, seq_dur, samples_per_track)
        train_loss = trainer.train_epoch(train, table)
        valid_loss = trainer.validate(valid, valid_chunk)
        scheduler.step(valid_loss)
        trainer.lr = float(shim.param_groups[0]["lr"])
        hist["train_loss_history"].append(train_loss)
        hist["valid_loss_history"].append(valid_loss)
        stop = es.step(valid_loss)
        is_best = valid_loss == es.best
        if is_best:
            hist["best_epoch"] = epoch
        hist["train_time_history"].append(time.time() - end)
        hist.update(epochs_trained=epoch, best_loss=es.best, num_bad_epochs=es.num_bad_epochs)
        if model_path is not None:
            state_dict, optimizer = trainer.checkpoint_state()
            torch.save({"epoch": epoch + 1, "state_dict": state_dict, "best_loss": es.best, "optimizer": optimizer,
                        "scheduler": scheduler.state_dict()}, os.path.join(model_path, CHECKPOINT))
            if is_best:
                torch.save(state_dict, os.path.join(model_path, WEIGHTS))
            args = dict(trainer.model_args(), seq_dur=seq_dur, batch_size=batch_size, samples_per_track=samples_per_track,
                        seed=seed, epochs=epochs, patience=patience, lr_decay_patience=lr_decay_patience,
                        lr_decay_gamma=lr_decay_gamma, model_path=str(model_path))
            with open(os.path.join(model_path, RESULTS), "w") as outfile:
                outfile.write(json.dumps(dict(hist, args=args), indent=4, sort_keys=True))
        if not quiet:
            print(f"epoch {epoch}: train_loss {train_loss:.6f} valid_loss {valid_loss:.6f} lr {trainer.lr:.3g} "
                  f"({hist['train_time_history'][-1]:.1f} s){' best' if is_best else ''}", flush=True)
        if stop:
            if not quiet:
                print("Apply Early Stopping")
            break
    return hist


def main(argv=None) -> dict:
    """``python -m xumx_slicq_amd.training``: ``training_main`` (training.py:157-556) for a directory of stems in the
    MUSDB18-HQ layout.  The reference's flag names and defaults; ``--root`` replaces ``--musdb-root``, ``--valid`` names the
    validation tracks (musdb's own train / valid split list is part of the musdb package, which is not a dependency),
    ``--storage`` and ``--precision`` are additions."""
    import argparse
    from .data import DeviceDataset
    from .model import Unmix
    from .statistics import get_statistics
    from .transforms import ComplexNorm, NSGTBase, make_filterbanks
    ap = argparse.ArgumentParser(description="xumx-sliCQ-V2 Trainer (MI355X)")
    ap.add_argument("--root", required=True, help="<root>/<track>/{vocals,drums,bass,other}.wav")
    ap.add_argument("--valid", required=True, help="comma-separated names of the validation tracks")
    ap.add_argument("--model-path", required=True)
    ap.add_argument("--samples-per-track", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--patience", type=int, default=1000)
    ap.add_argument("--lr-decay-patience", type=int, default=80)
    ap.add_argument("--lr-decay-gamma", type=float, default=0.3)
    ap.add_argument("--weight-decay", type=float, default=0.00001)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--sdr-mcoef", type=float, default=-1.0)
    ap.add_argument("--realtime", action="store_true", default=False)
    ap.add_argument("--seq-dur", type=float, default=2.0)
    ap.add_argument("--fscale", choices=("bark", "mel"), default="bark")
    ap.add_argument("--fbins", type=int, default=262)
    ap.add_argument("--fmin", type=float, default=32.9)
    ap.add_argument("--storage", choices=("pcm16", "fp32"), default="pcm16")
    ap.add_argument("--precision", choices=("fp32", "bf16", "bf16x6"), default="fp32")
    ap.add_argument("--quiet", action="store_true", default=False)
    a = ap.parse_args(argv)
    device = torch.device("cuda")
    valid_names = [v for v in a.valid.split(",") if v]
    names = sorted(d for d in os.listdir(a.root) if os.path.isdir(os.path.join(a.root, d)))
    missing = [v for v in valid_names if v not in names]
    if missing or not valid_names:
        raise SystemExit(f"--valid: {missing or 'no track named'} (tracks under {a.root}: {len(names)})")
    train = DeviceDataset.from_directory(a.root, [n for n in names if n not in valid_names], storage=a.storage, device=device)
    valid = DeviceDataset.from_directory(a.root, valid_names, storage=a.storage, device=device)
    nsgt_base = NSGTBase(a.fscale, a.fbins, a.fmin, fs=train.sample_rate, device=device)
    nsgt, insgt = make_filterbanks(nsgt_base, sample_rate=train.sample_rate)
    encoder = (nsgt.to(device), insgt.to(device), ComplexNorm().to(device))
    jagged, _ = nsgt_base.predict_input_size(a.batch_size, 2, a.seq_dur)
    means = stds = None
    if not os.path.exists(os.path.join(a.model_path, CHECKPOINT)):          # data whitening (training.py:371-375)
        means, stds = get_statistics(encoder, (x[0] for i in range(len(train)) for x, _ in train.pieces(i, int(train.lengths[i]))))
    unmix = Unmix(encoder[2](jagged), realtime=a.realtime, input_means=means, input_scales=stds).to(device)
    trainer = Trainer(unmix, encoder, lr=a.lr, weight_decay=a.weight_decay, device=device, precision=a.precision,
                      sdr_mcoef=a.sdr_mcoef)
    return trainer.fit(train, valid, a.epochs, batch_size=a.batch_size, seq_dur=a.seq_dur, samples_per_track=a.samples_per_track,
                       seed=a.seed, patience=a.patience, lr_decay_patience=a.lr_decay_patience, lr_decay_gamma=a.lr_decay_gamma,
                       model_path=a.model_path, quiet=a.quiet)


if __name__ == "__main__":
    main()
