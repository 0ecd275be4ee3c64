"""The table / judge helper of the float64 parity tests (tests/test_ref64_gpu.py, tests/test_ref64_mel_gpu.py, tests/test_ref64_train_gpu.py, tests/test_ref64_stress_gpu.py).

TEST INFRASTRUCTURE (see oracle/__init__.py).  One rule for every stage:  e_gpu <= M * E,  e_gpu the kernels' error against
oracle/ref64.py, E the LARGEST error of the fp32 CPU oracle over the members of the stage on the same input, both by
``ref64.rel_err``; M per stage, a power of two, at most ``M_CAP`` for fp32-grade arithmetic.  ``Tables`` prints every
comparison, keeps it, and writes what it kept as JSON when XSQ_REF64_TABLES is set: a file name (the module that ran last
wins) or an existing directory (every module writes ``<name>.json`` into it).
"""
from __future__ import annotations

import json
import os

import numpy as np

M_CAP = 16


class Tables:
    def __init__(self, name: str, M: dict):
        self.name, self.M, self.tables = name, M, {}

    def judge(self, stage, case, e_gpu, e_cpu, labels, full_table=False, arm=None, localise=False):
        """Print the table, record it, and return the failures of  e_gpu <= M * E  (E = largest e_cpu, per metric).  ``localise``: for
        a stage whose e_cpu varies widely over its members, the RMS metric of member i is judged against  max(e_cpu[i], median e_cpu)
        instead of the largest (the maximum alone would let the kernels be  largest / median  times worse than the oracle on a typical
        member); the max metric keeps the largest e_cpu."""
        M = self.M
        key = f"{stage}/{arm}" if f"{stage}/{arm}" in M else stage
        bound = M[key]
        (g_rms, g_max), (c_rms, c_max) = e_gpu, e_cpu
        g_rms, g_max, c_rms, c_max = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (g_rms, g_max, c_rms, c_max))
        assert g_rms.shape == g_max.shape == c_rms.shape == c_max.shape == (len(labels),), (g_rms.shape, c_rms.shape, len(labels))
        E_rms, E_max = float(c_rms.max()), float(c_max.max())
        E_loc = np.maximum(c_rms, np.median(c_rms)) if localise else E_rms
        ratio = np.maximum(g_rms / E_loc, g_max / E_max)
        w = int(np.argmax(ratio))
        print(f"\n[{stage}] {case}: E_rms {E_rms:.3e} E_max {E_max:.3e}; worst e_gpu / E = {ratio[w]:.2f} at {labels[w]} (M = {bound})")
        print("  index / class                      e_gpu rms   e_gpu max   e_cpu rms   e_cpu max   ratio")
        for i, lab in enumerate(labels):
            print(f"  {lab:34s} {g_rms[i]:.3e}   {g_max[i]:.3e}   {c_rms[i]:.3e}   {c_max[i]:.3e}   {ratio[i]:.2f}")
        rec = {"M_key": key, "E_rms": E_rms, "E_max": E_max, "worst_ratio": float(ratio[w]), "worst_at": labels[w],
               "worst_e_gpu_rms": float(g_rms.max()), "worst_e_gpu_max": float(g_max.max())}
        if localise:
            rec["E_rms_median"] = float(np.median(c_rms))
        if full_table:
            rec["table"] = {"label": list(labels), "e_gpu_rms": g_rms.tolist(), "e_gpu_max": g_max.tolist(),
                            "e_cpu_rms": c_rms.tolist(), "e_cpu_max": c_max.tolist()}
        self.tables.setdefault(stage, {})[case] = rec
        bad = [f"{labels[i]}: e_gpu rms {g_rms[i]:.3e} max {g_max[i]:.3e} = {ratio[i]:.2f} x E" for i in np.nonzero(~(ratio <= bound))[0]]     # (a NaN fails)
        return bad, float(ratio[w])

    def record(self, stage, case, rec):
        """A comparison judged elsewhere (``rec`` carries at least ``worst_ratio``; ``M_key`` defaults to the stage)."""
        self.tables.setdefault(stage, {})[case] = rec

    def dump(self):
        path = os.environ.get("XSQ_REF64_TABLES")
        if not path:
            return
        if os.path.isdir(path):
            path = os.path.join(path, self.name + ".json")
        worst = {}
        for stage, cases in self.tables.items():
            for case, rec in cases.items():
                key = rec.get("M_key", stage)
                if rec["worst_ratio"] > worst.get(key, {"worst_ratio": -1.0})["worst_ratio"]:
                    worst[key] = {"worst_ratio": rec["worst_ratio"], "case": case, "at": rec.get("worst_at", ""), "M": self.M.get(key)}
        with open(path, "w") as f:
            json.dump({"M": worst, "tables": self.tables}, f, indent=0, sort_keys=True)
