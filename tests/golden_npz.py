"""Golden .npz fixtures under the repository's 1 MiB per-file limit.

An archive whose arrays would exceed PART_BYTES is stored as <name>.npz plus <name>.part1.npz, <name>.part2.npz, ...:
the keys in their original order, cut into consecutive runs.  load() merges the parts back into one mapping with the
`files` / `[key]` interface of np.load's NpzFile; save() (tools/gen_golden.py) writes them."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PART_BYTES = 900 * 1024


class Golden(dict):
    @property
    def files(self):
        return list(self)


def _parts(path):
    return sorted(glob.glob(path[:-len('.npz')] + '.part*.npz'), key=lambda p: int(p.rsplit('.part', 1)[1][:-len('.npz')]))


def load(name):
    """tests/golden/<name> (a file name ending in .npz, or an absolute path) with all its parts."""
    path = name if os.path.isabs(name) else os.path.join(GOLDEN, name)
    d = Golden()
    for p in [path] + _parts(path):
        with np.load(p) as z:
            for k in z.files:
                assert k not in d, (p, k)
                d[k] = z[k]
    return d


def save(path, **arrays):
    """np.savez, cut into parts of at most PART_BYTES of array data (a single larger array keeps a part of its own)."""
    for p in _parts(path):
        os.remove(p)
    runs, size = [[]], 0
    for k, v in arrays.items():
        n = np.asarray(v).nbytes
        if runs[-1] and size + n > PART_BYTES:
            runs.append([])
            size = 0
        runs[-1].append(k)
        size += n
    for i, keys in enumerate(runs):
        p = path if i == 0 else f'{path[:-len(".npz")]}.part{i}.npz'
        np.savez(p, **{k: arrays[k] for k in keys})
