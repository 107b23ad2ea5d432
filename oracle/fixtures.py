"""Golden fixtures (tests/golden/*.npz).  An archive above the repository's 1 MiB file limit is stored as numbered pieces
<stem>.0.npz, <stem>.1.npz, ... (whole arrays, the keys split between them); load() reads either form as one mapping."""
import io
import os

import numpy as np

LIMIT = 1 << 20


def load(path):
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    stem, out, i = path[:-len(".npz")], {}, 0
    while os.path.exists(f"{stem}.{i}.npz"):
        with np.load(f"{stem}.{i}.npz", allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
        i += 1
    if i == 0:
        raise FileNotFoundError(path)
    return out


def save(path, arrays, limit=LIMIT):
    """np.savez_compressed(path, **arrays), as pieces of less than `limit` bytes each when one archive would exceed it."""
    stem = path[:-len(".npz")]
    for f in [path] + [f"{stem}.{i}.npz" for i in range(64)]:
        if os.path.exists(f):
            os.remove(f)

    def packed(keys):
        b = io.BytesIO()
        np.savez_compressed(b, **{k: arrays[k] for k in keys})
        return b.getvalue()
    if len(packed(arrays)) < limit:
        np.savez_compressed(path, **arrays)
        return [path]
    pieces, cur = [], []
    for k in arrays:
        if cur and len(packed(cur + [k])) >= limit:
            pieces.append(cur); cur = []
        cur.append(k)
    pieces.append(cur)
    paths = []
    for i, keys in enumerate(pieces):
        data = packed(keys)
        assert len(data) < limit, (path, keys)
        paths.append(f"{stem}.{i}.npz")
        with open(paths[-1], "wb") as f:
            f.write(data)
    return paths
