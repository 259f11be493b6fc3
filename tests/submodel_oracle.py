"""The numpy restatement of sub-model aggregation (examples/model_search/{heterofl,fjord,fedrolex,anycostfl}:
Algorithm.aggregation), one fp32 operation at a time.

For every key of the global model G, in G's order: a key with neither "weight" nor "bias" in it is copied
from G (dtype and bits kept).  Any other key has a prefix rank r from its number of dims and the rule, and
per element

    acc = g
    for k in arrival order, if client k covers the element:  acc = acc + x_k    (fp32 add)
    out = (acc - g) / float(max(count, 1))                                      (fp32 sub, IEEE fp32 division)

Client k covers the elements whose first r indices are below its own first r extents.  numpy's float32
`+`, `-` and `/` on arrays are single IEEE operations, so the loop below is the contract, not a bound.
"""

from __future__ import annotations

from collections import OrderedDict

import numpy as np

RANKS = {"heterofl": {4: 2, 2: 2, 1: 1}, "fedrolex": {4: 2, 2: 2, 1: 1, 3: 3}}


def participates(name: str) -> bool:
    return "weight" in name or "bias" in name


def rank_of(rule: str, ndim: int) -> int:
    return RANKS[rule].get(ndim, 0)


def aggregate(global_model, clients, rule: str):
    """``global_model``: name -> ndarray; ``clients``: list of name -> ndarray.  Returns
    (name -> ndarray, name -> int32 count array for the participating keys)."""
    out, counts = OrderedDict(), OrderedDict()
    with np.errstate(all="ignore"):
        for name, g in global_model.items():
            g = np.asarray(g)
            if not participates(name):
                out[name] = g.copy()
                continue
            assert g.dtype == np.float32, name
            r = rank_of(rule, g.ndim)
            acc = g.copy()
            count = np.zeros(g.shape, dtype=np.int32)
            if r:
                for client in clients:
                    x = np.asarray(client[name])
                    assert x.dtype == np.float32 and x.shape[r:] == g.shape[r:], name
                    box = tuple(slice(0, s) for s in x.shape[:r])
                    acc[box] = acc[box] + x
                    count[box] += 1
            out[name] = ((acc - g) / np.maximum(count, 1).astype(np.float32)).astype(np.float32)
            counts[name] = count
    return out, counts
