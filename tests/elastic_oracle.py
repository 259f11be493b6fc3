"""The numpy restatement of elastic sub-model aggregation (examples/model_search/sysheterofl:
Algorithm.aggregation), one fp32 operation at a time.

For every key of the global model G, in G's order: the key has a rank from its number of dims (4, 2 and 1
are their own rank, any other is 0; with update_track false a 1-D key with "running" or "tracked" in its name
is 0 too).  A client takes part in a key of rank >= 1 that it holds, and covers the elements whose indices
are all below its own extents.  Per element

    acc = g
    for k in arrival order, if client k holds the key and covers the element:  acc = acc + x_k    (fp32 add)
    out = (acc - g) / float(max(count, 1))                                     (fp32 sub, IEEE fp32 division)

A float32 key of rank 0, or one nobody holds, is all (g - g) / 1.  A key of G that is not float32 gives
float32 zeros if it is an integer key whose number of dims is not 1, 2 or 4 (an integer g - g is exactly 0),
and is refused otherwise.  numpy's float32 `+`, `-` and `/` on arrays are single IEEE operations, so the
loop below is the contract, not a bound.
"""

from __future__ import annotations

from collections import OrderedDict

import numpy as np


def rank_of(name: str, ndim: int, update_track: bool = True) -> int:
    if ndim not in (4, 2, 1):
        return 0
    if ndim == 1 and not update_track and ("running" in name or "tracked" in name):
        return 0
    return ndim


def aggregate(global_model, clients, update_track: bool = True):
    """``global_model``: name -> ndarray; ``clients``: list of name -> ndarray (keys may be missing).
    Returns (name -> float32 ndarray, name -> int32 count array)."""
    out, counts = OrderedDict(), OrderedDict()
    with np.errstate(all="ignore"):
        for name, g in global_model.items():
            g = np.asarray(g)
            count = np.zeros(g.shape, dtype=np.int32)
            counts[name] = count
            if g.dtype != np.float32:
                if not (np.issubdtype(g.dtype, np.integer) and g.ndim not in (1, 2, 4)):
                    raise ValueError(f"{name}: {g.dtype} with {g.ndim} dims")
                out[name] = np.zeros(g.shape, dtype=np.float32)
                continue
            acc = g.copy()
            if rank_of(name, g.ndim, update_track):
                for client in clients:
                    if name not in client:
                        continue
                    x = np.asarray(client[name])
                    assert x.dtype == np.float32 and x.ndim == g.ndim, name
                    assert all(s <= d for s, d in zip(x.shape, g.shape)), name
                    box = tuple(slice(0, s) for s in x.shape)
                    acc[box] = acc[box] + x
                    count[box] += 1
            out[name] = ((acc - g) / np.maximum(count, 1).astype(np.float32)).astype(np.float32)
    return out, counts
