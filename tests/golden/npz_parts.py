"""Golden arrays stored as NAME.0.npz, NAME.1.npz, ... so that no committed file exceeds 1 MiB.
load(NAME) returns the merged {key: array} dict; save(NAME, arrays) writes the parts (arrays in
order, a new part whenever the next one would not fit; an array that does not fit a part on its
own is cut along axis 0 into pieces `key#i`, which load() joins again)."""
import glob
import io
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 960 << 10  # bytes per part, below the 1 MiB limit of a committed file


def _parts(name):
    found = glob.glob(os.path.join(HERE, name + ".*.npz"))
    return sorted(found, key=lambda p: int(p.rsplit(".", 2)[1]))


def load(name):
    paths = _parts(name)
    if not paths:
        raise FileNotFoundError(os.path.join(HERE, name + ".0.npz"))
    flat = {}
    for p in paths:
        with np.load(p) as d:
            flat.update({k: d[k] for k in d.files})
    out, pieces = {}, {}
    for k, a in flat.items():
        m = re.fullmatch(r"(.*)#(\d+)", k)
        if m:
            pieces.setdefault(m.group(1), {})[int(m.group(2))] = a
        else:
            out[k] = a
    for k, ps in pieces.items():
        out[k] = np.concatenate([ps[i] for i in range(len(ps))], axis=0)
    return out


def _size(key, a):
    b = io.BytesIO()
    np.savez_compressed(b, **{key: a})
    return len(b.getvalue())


def save(name, arrays):
    items = []
    for k, a in arrays.items():
        a = np.asarray(a)
        n = -(-_size(k, a) // LIMIT)
        while n > 1 and max(_size(k, c) for c in np.array_split(a, n, axis=0)) > LIMIT:
            n += 1
        if n == 1:
            items.append((k, a))
        else:
            items += [(f"{k}#{i}", c) for i, c in enumerate(np.array_split(a, n, axis=0))]
    for p in _parts(name):
        os.remove(p)
    part, cur, used = 0, {}, 0
    for k, a in items:
        s = _size(k, a)
        if cur and used + s > LIMIT:
            np.savez_compressed(os.path.join(HERE, f"{name}.{part}.npz"), **cur)
            part, cur, used = part + 1, {}, 0
        cur[k] = a
        used += s
    np.savez_compressed(os.path.join(HERE, f"{name}.{part}.npz"), **cur)
