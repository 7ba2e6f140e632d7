"""Fixtures of the suite.  A fixture too large for one committed file (1 MiB) is stored in parts:
NAME.npz, NAME.part1.npz, NAME.part2.npz, ...; every array lies whole in one part."""
import os

import numpy as np

PART_MAX_BYTES = 1 << 20


def _part(path, k):
    return path if k == 0 else path[:-4] + f".part{k}.npz"


def load_parts(path):
    """{name: array} of NAME.npz and the parts beside it."""
    out, k = {}, 0
    while os.path.exists(_part(path, k)):
        with np.load(_part(path, k)) as d:
            out.update({n: d[n] for n in d.files})
        k += 1
    if not out:
        raise FileNotFoundError(path)
    return out


def save_parts(path, **arrays):
    """np.savez_compressed into as many parts as keep every file within PART_MAX_BYTES (arrays in
    the given order; a part is closed when the next array would take it over the limit)."""
    assert path.endswith(".npz")
    k = 0
    while os.path.exists(_part(path, k)):  # parts of an earlier, longer fixture
        os.remove(_part(path, k))
        k += 1
    k, cur = 0, {}
    for name, a in arrays.items():
        np.savez_compressed(_part(path, k), **cur, **{name: a})
        if cur and os.path.getsize(_part(path, k)) > PART_MAX_BYTES:
            np.savez_compressed(_part(path, k), **cur)
            k, cur = k + 1, {}
            np.savez_compressed(_part(path, k), **{name: a})
        if os.path.getsize(_part(path, k)) > PART_MAX_BYTES:
            raise ValueError(f"{name} alone does not fit a part of {PART_MAX_BYTES} bytes")
        cur[name] = a
    return k + 1
