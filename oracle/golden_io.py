"""Golden fixtures on disk: `<name>.npz`, or -- when that one file would pass the size
limit of a committed file -- `<name>.0.npz`, `<name>.1.npz`, ... holding the same arrays.

A split fixture keeps its arrays in order, as many per file as fit; an array too large
for one file is cut into flat pieces `<key>//<i>` with its shape under `<key>//shape`.
`load` gives back exactly the arrays `save` was given (same dtype, shape and bytes)."""
from __future__ import annotations

import glob
import io
import os

import numpy as np

LIMIT = 1_000_000        # bytes of one fixture file (under 1 MiB with some room)
PIECE = 3 * LIMIT // 4   # raw bytes of one piece of a cut array (deflate never grows it much)


def _packed(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save(golden, name, arrays):
    """Write the fixture `name` under `golden`; returns the files written."""
    for old in [os.path.join(golden, f"{name}.npz")] + \
            glob.glob(os.path.join(golden, f"{name}.[0-9]*.npz")):
        if os.path.exists(old):
            os.remove(old)
    whole = _packed(arrays)
    if len(whole) <= LIMIT:
        files = [whole]
    else:
        pieces = []
        for k, a in arrays.items():
            a = np.asarray(a)
            if a.nbytes <= PIECE:
                pieces.append((k, a))
                continue
            flat = np.ascontiguousarray(a).reshape(-1)
            per = max(1, PIECE // a.itemsize)
            pieces.append((f"{k}//shape", np.asarray(a.shape, dtype=np.int64)))
            pieces += [(f"{k}//{i}", flat[o:o + per])
                       for i, o in enumerate(range(0, flat.size, per))]
        files, cur = [], {}
        for k, a in pieces:
            if cur and len(_packed({**cur, k: a})) > LIMIT:
                files.append(_packed(cur))
                cur = {}
            cur[k] = a
        files.append(_packed(cur))
    paths = []
    for i, blob in enumerate(files):
        assert len(blob) <= LIMIT, (name, i, len(blob))
        p = os.path.join(golden, f"{name}.npz" if len(files) == 1 else f"{name}.{i}.npz")
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
    return paths


def load(golden, name):
    """The fixture `name` as a dict of arrays."""
    one = os.path.join(golden, f"{name}.npz")
    if os.path.exists(one):
        paths = [one]
    else:
        paths = sorted(glob.glob(os.path.join(golden, f"{name}.[0-9]*.npz")),
                       key=lambda p: int(os.path.basename(p).split(".")[-2]))
        if not paths:
            raise FileNotFoundError(one)
    raw = {}
    for p in paths:
        with np.load(p) as d:
            raw.update({k: d[k] for k in d.files})
    out = {}
    for k, a in raw.items():
        if "//" not in k:
            out[k] = a
        elif k.endswith("//shape"):
            key = k[:-len("//shape")]
            n = sum(1 for q in raw if q.startswith(key + "//")) - 1
            out[key] = np.concatenate([raw[f"{key}//{i}"] for i in range(n)]).reshape(tuple(a))
    return out
