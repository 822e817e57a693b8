"""Golden vectors under tests/golden/ as .npz files of at most PART_BYTES each.  A vector that would be larger is stored
as ``<name>.part<k>.npz`` files; an array too large for one part is cut along its first axis into ``<key>@<i>`` pieces.
``load(path)`` gives the same arrays either way.  Test infrastructure only."""
import glob
import io
import os
import re

import numpy as np

PART_BYTES = 960 * 1024      # below the 1 MiB limit for a committed file


class Golden(dict):
    """the arrays of one golden vector: g[key], key in g, g.files (as np.load's NpzFile offers them)"""

    @property
    def files(self):
        return list(self)


def _parts(path):
    stem = path[:-len(".npz")]
    return sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))


def load(path):
    if os.path.exists(path):
        return np.load(path)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    pieces, out = {}, Golden()
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                key, _, i = k.partition("@")
                if i:
                    pieces.setdefault(key, {})[int(i)] = z[k]
                else:
                    out[key] = z[k]
    for key, d in pieces.items():
        out[key] = np.concatenate([d[i] for i in range(len(d))], axis=0)
    return out


def _compressed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(path, arrays):
    """np.savez_compressed(path, **arrays), or the part files when that would exceed PART_BYTES (old parts removed)"""
    stem = path[:-len(".npz")]
    for p in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(p)
    if _compressed_size(arrays) <= PART_BYTES:
        np.savez_compressed(path, **arrays)
        return [path]
    items = []                      # (key, array) with every array small enough for a part of its own
    for k, a in arrays.items():
        n = 1
        while a.ndim and n <= a.shape[0] and any(_compressed_size({"a": c}) > PART_BYTES
                                                  for c in np.array_split(a, n, axis=0)):
            n += 1
        if n == 1:
            items.append((k, a))
        else:
            items += [(f"{k}@{i}", c) for i, c in enumerate(np.array_split(a, n, axis=0))]
    groups, cur = [], {}
    for k, a in items:
        if cur and _compressed_size(dict(cur, **{k: a})) > PART_BYTES:
            groups.append(cur)
            cur = {}
        cur[k] = a
    groups.append(cur)
    written = []
    for i, g in enumerate(groups):
        written.append(f"{stem}.part{i}.npz")
        np.savez_compressed(written[-1], **g)
    return written
