"""Storage of the fixtures under ``tests/golden/``: compressed ``.npz`` files of at most 1 MiB each.

A fixture whose arrays do not fit into one such file is split by key into ``<name>.part0.npz``, ``<name>.part1.npz``, ...
(every array whole, keys in their original order); ``load`` reads either form and returns the same mapping.
"""
from __future__ import annotations

import glob
import io
import os
import re

import numpy as np

LIMIT = 1 << 20           # bytes per committed file


def _npz_bytes(arrays):
    b = io.BytesIO()
    np.savez_compressed(b, **arrays)
    return b.getvalue()


def _part_paths(path):
    stem = path[:-len(".npz")]
    parts = glob.glob(glob.escape(stem) + ".part*.npz")
    return sorted((p for p in parts if re.fullmatch(r"\d+", p[len(stem) + 5:-4])), key=lambda p: int(p[len(stem) + 5:-4]))


def save(path, **arrays):
    """Write ``arrays`` as ``path`` (``<name>.npz``), or as its parts when one file would exceed LIMIT; returns the paths."""
    assert path.endswith(".npz"), path
    parts, cur = [], {}
    for k, v in arrays.items():
        if cur and len(_npz_bytes({**cur, k: v})) > LIMIT:
            parts.append(cur)
            cur = {}
        cur[k] = v
    parts.append(cur)
    blobs = [_npz_bytes(p) for p in parts]
    if max(len(b) for b in blobs) > LIMIT:
        raise ValueError(f"{path}: an array alone exceeds {LIMIT} bytes compressed")
    for old in _part_paths(path) + ([path] if os.path.exists(path) else []):
        os.remove(old)                       # no stale file of the other form
    out = [path] if len(blobs) == 1 else [path[:-len(".npz")] + f".part{i}.npz" for i in range(len(blobs))]
    for p, b in zip(out, blobs):
        with open(p, "wb") as f:
            f.write(b)
    return out


class Fixture(dict):
    """The arrays of a fixture by key; ``files`` lists the keys in their stored order (as ``np.load(...).files`` does)."""

    @property
    def files(self):
        return list(self)


def load(path):
    """The fixture ``path`` (``<name>.npz``) stored whole or in parts."""
    if os.path.exists(path):
        return np.load(path)
    parts = _part_paths(path)
    if not parts:
        raise FileNotFoundError(path)
    out = Fixture()
    for p in parts:
        with np.load(p) as z:
            out.update((k, z[k]) for k in z.files)
    return out
