"""Reading and writing the golden sets under tests/golden/.

A set is one compressed .npz, or, where its arrays do not fit one file of
PART_LIMIT bytes, a first file <name>.npz and continuation files
<name>.part2.npz, <name>.part3.npz, ... holding the remaining arrays; load()
gives the whole set as one dict either way. No array is altered: the parts
hold the arrays exactly as a single file would.
"""
from __future__ import annotations

import glob
import io
import os

import numpy as np

PART_LIMIT = 1_000_000  # bytes per stored file (the repository keeps every file under 1 MiB)


def _packed(arrays: dict) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save(path: str, **arrays) -> list[str]:
    """Store the arrays in order as path (…/<name>.npz) and as many
    continuation files as PART_LIMIT asks for; returns the files written."""
    stem = path[:-len(".npz")]
    parts, cur = [], {}
    for k, v in arrays.items():
        if cur and len(_packed({**cur, k: v})) > PART_LIMIT:
            parts.append(cur)
            cur = {}
        cur[k] = v
    parts.append(cur)
    for old in glob.glob(glob.escape(stem) + ".part*.npz"):
        os.remove(old)
    written = []
    for i, part in enumerate(parts, 1):
        data = _packed(part)
        if len(data) > PART_LIMIT:
            raise ValueError(f"{list(part)} alone exceeds {PART_LIMIT} bytes")
        name = path if i == 1 else f"{stem}.part{i}.npz"
        with open(name, "wb") as f:
            f.write(data)
        written.append(name)
    return written


def load(path: str) -> dict:
    """Every array of the set stored at path (…/<name>.npz) and its
    continuation files, by name."""
    stem = path[:-len(".npz")]
    out = {}
    for name in [path] + sorted(glob.glob(glob.escape(stem) + ".part*.npz")):
        with np.load(name, allow_pickle=False) as z:
            for k in z.files:
                if k in out:
                    raise ValueError(f"{name}: array {k!r} is stored twice in the set")
                out[k] = z[k]
    return out
