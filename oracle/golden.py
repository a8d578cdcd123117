"""Fixture files under tests/golden/: one case = ``<name>.npz`` plus, when its arrays exceed SHARD_BYTES, the shards
``<name>.1.npz``, ``<name>.2.npz``, ... (every committed file stays well under 1 MiB).  An array larger than a shard is
stored in pieces along axis 0, keys ``<key>@0``, ``<key>@1``, ...; ``load`` puts it back together.

Test infrastructure only -- see oracle/__init__.py.
"""
import os

import numpy as np

SHARD_BYTES = 768 << 10      # uncompressed bytes per file: a compressed shard can never reach 1 MiB


def save(directory, name, arrays):
    pieces = {}
    for k, a in arrays.items():
        a = np.asarray(a)
        n = 1 if a.nbytes <= SHARD_BYTES else -(-a.nbytes // SHARD_BYTES)
        if n == 1:
            pieces[k] = a
        else:
            for i, p in enumerate(np.array_split(a, n)):
                pieces['%s@%d' % (k, i)] = p
    shards, size = [{}], 0
    for k, a in pieces.items():
        if shards[-1] and size + a.nbytes > SHARD_BYTES:
            shards.append({})
            size = 0
        shards[-1][k] = a
        size += a.nbytes
    i = 1
    while os.path.exists(os.path.join(directory, '%s.%d.npz' % (name, i))):      # (shards of an earlier, larger case)
        os.remove(os.path.join(directory, '%s.%d.npz' % (name, i)))
        i += 1
    for i, s in enumerate(shards):
        np.savez_compressed(os.path.join(directory, name + ('.npz' if i == 0 else '.%d.npz' % i)), **s)


def load(directory, name):
    d, i = dict(np.load(os.path.join(directory, name + '.npz'))), 1
    while os.path.exists(os.path.join(directory, '%s.%d.npz' % (name, i))):
        d.update(np.load(os.path.join(directory, '%s.%d.npz' % (name, i))))
        i += 1
    split = {}
    for k in [k for k in d if '@' in k]:
        base, j = k.rsplit('@', 1)
        split.setdefault(base, {})[int(j)] = d.pop(k)
    for base, parts in split.items():
        d[base] = np.concatenate([parts[j] for j in range(len(parts))])
    return d
