"""Array fixtures of tests/golden stored in parts, so that no committed file passes 1 MiB.

<name>.part<i>.npz (i = 0, 1, ...) hold, in order, the pieces of one set of arrays: an array found in
several parts is the concatenation of its pieces along axis 0, any other is taken from the one part
that holds it.  load_npz(name) gives back the arrays save_npz(name, arrays) was handed, bit for bit.
"""
import glob
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FILE_BYTES = 1 << 20
_RAW_PART_BYTES = MAX_FILE_BYTES - (64 << 10)      # uncompressed bytes per part: the .npz stays below the limit


def part_paths(name, golden=GOLDEN):
    paths = glob.glob(os.path.join(golden, f"{glob.escape(name)}.part*.npz"))
    key = {p: re.search(r"\.part(\d+)\.npz$", p) for p in paths}
    return sorted((p for p in paths if key[p]), key=lambda p: int(key[p].group(1)))


def load_npz(name, golden=GOLDEN):
    """{array name: array} of the fixture `name` (tests/golden/<name>.part*.npz)"""
    paths = part_paths(name, golden)
    if not paths:
        raise FileNotFoundError(f"no {name}.part*.npz in {golden}")
    pieces = {}
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                pieces.setdefault(k, []).append(z[k])
    return {k: v[0] if len(v) == 1 else np.concatenate(v) for k, v in pieces.items()}


def save_npz(name, arrays, golden=GOLDEN):
    """Writes `arrays` as <name>.part*.npz (compressed), every file below MAX_FILE_BYTES."""
    items = []
    for k, a in arrays.items():
        a = np.asarray(a)
        if a.ndim and a.nbytes > _RAW_PART_BYTES:
            items += [(k, c) for c in np.array_split(a, -(-a.nbytes // _RAW_PART_BYTES))]
        else:
            items.append((k, a))
    parts, size = [{}], 0
    for k, a in items:
        if k in parts[-1] or (parts[-1] and size + a.nbytes > _RAW_PART_BYTES):
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    for p in part_paths(name, golden):
        os.remove(p)
    for i, part in enumerate(parts):
        path = os.path.join(golden, f"{name}.part{i}.npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < MAX_FILE_BYTES, path
