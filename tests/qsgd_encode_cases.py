"""The QSGD-quantizer cases and their reference-generated fixtures (tests/golden/qsgd_encode_cases.json, .npz).

A case is one state (name -> tensor, fp32 or int64, in ``state_dict()`` order), a quantization level and a
draw seed.  The generator (tests/golden/make_golden_qsgd_encode.py) runs the reference's own
``Processor._process_layer`` on every entry with ``random.random`` replaced by a feed of the project's draws
(tests/qsgd_encode_oracle.py: ``draws``; the entry at row offset ``at`` takes the draws of the row elements
[at, at + numel)) and records the bytes it produced.  Every comparison against them is byte for byte.
"""

from __future__ import annotations

import functools
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from tests import prune_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON_PATH = os.path.join(GOLDEN, "qsgd_encode_cases.json")
NPZ_PATH = os.path.join(GOLDEN, "qsgd_encode_small.npz")


def recipes():
    """name, what the state is, the seed of its values, the level, the seed of the draws."""
    def one(name, state, seed, level, draw_seed):
        return {"name": name, "state": state, "seed": seed, "level": level, "draw_seed": draw_seed}

    return [
        one("toy_l2", "toy", 6101, 2, 11),
        one("toy_l64", "toy", 6102, 64, 12),
        one("toy_l128", "toy", 6103, 128, (1 << 64) - 3),
        one("lenet5_l64", "lenet5", 6104, 64, 14),
        one("special_l2", "special", 6105, 2, 15),
        one("special_l64", "special", 6105, 64, 16),
        one("special_l128", "special", 6105, 128, 17),
    ]


def _f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def special_state(seed: int) -> "OrderedDict[str, np.ndarray]":
    """Entries of special values.  The shapes cover 0-d, 1-d and 4-d; the element counts are odd so that the
    entries start at every row offset mod 4 and mod 2 (the draws pair the elements of the row)."""
    rng = np.random.default_rng(seed)
    normal = lambda n, scale=0.1: (rng.standard_normal(n) * scale).astype(np.float32)  # noqa: E731
    st = OrderedDict()
    # +-0 among ordinary values
    a = normal(37)
    a[::3] = 0.0
    a[1::6] = -0.0
    st["zeros.signed"] = a
    # subnormals under a subnormal maximum
    mant = rng.integers(1, 1 << 22, 41).astype(np.uint32)
    mant[7] = 0x007FFFFF
    mant[::5] |= 0x80000000
    st["subnormal.max_subnormal"] = _f32(mant).reshape(41)
    # a maximum near 3e38 (0x7f61b1e6 = 3.0e38), over values across the whole exponent range
    a = (normal(45, 1.0) * np.float32(2.0) ** rng.integers(-120, 120, 45).astype(np.float32)).astype(np.float32)
    a[13] = _f32([0x7F61B1E6])[0]
    a[14] = _f32([0xFF61B1E5])[0]
    st["huge.max_3e38"] = a.reshape(3, 3, 5, 1)
    # the maximum is negative
    a = normal(29)
    a[11] = -1.5
    st["negative.max"] = a
    # x = |v| / m * tp below, at and above 2^-25 (lvl = -1 and p = 1 below it), m = 1
    tiny = [2.0**-40, -(2.0**-40), 2.0**-33, 2.0**-32, 2.0**-31, -(2.0**-31), 2.0**-30, 2.0**-26, 2.0**-25,
            -(2.0**-25), 2.0**-24, 1e-10, -1e-10, 1e-45, -1e-45, 2.0**-25 / 63, 2.0**-25 / 127, 3e-9, 6e-9, 1.0]
    st["tiny.x"] = np.asarray(tiny, dtype=np.float32)
    # the maximum first, last and repeated (with both signs)
    a = normal(23)
    a[0] = 0.75
    st["max.first"] = a
    a = normal(26)
    a[-1] = -0.75
    st["max.last"] = a.reshape(2, 13)
    a = normal(31)
    a[[2, 9, 30]] = 0.5
    a[[5, 17]] = -0.5
    st["max.repeated"] = a
    # values on the level grid: x lands on or beside an integer
    st["exact.levels"] = (np.arange(-63, 64, dtype=np.float32) / np.float32(64)).astype(np.float32)
    # one element; a 0-d entry; int64 entries: a 0-d counter, a vector with negatives and a value above 2^24
    st["single"] = np.asarray([-0.3], dtype=np.float32)
    st["scalar.float"] = np.asarray(0.7, dtype=np.float32)
    st["counter"] = np.asarray(1234, dtype=np.int64)
    st["ints"] = np.asarray([3, -7, 0, (1 << 24) + 1, -5, 100000, 1], dtype=np.int64)
    return st


def seeded_state(recipe) -> "OrderedDict[str, np.ndarray]":
    """The state of a recipe as numpy arrays (what the generator quantizes and the fixture records)."""
    if recipe["state"] == "special":
        return special_state(recipe["seed"])
    rng = np.random.default_rng(recipe["seed"])
    model = prune_cases.build(recipe["state"])
    st = OrderedDict()
    for key, t in model.state_dict().items():
        if t.dtype == torch.float32:
            a = (rng.standard_normal(t.numel()) * (1.0 if "running_var" in key else 0.1)).astype(np.float32)
            if "running_var" in key:
                a = np.abs(a) + np.float32(0.5)
            st[key] = a.reshape(tuple(t.shape))
        else:
            st[key] = np.asarray(int(rng.integers(1, 1000)), dtype=np.int64).reshape(tuple(t.shape))
    return st


@functools.lru_cache(maxsize=None)
def _load():
    with open(JSON_PATH) as f:
        meta = json.load(f)
    return meta, np.load(NPZ_PATH)


def case_ids():
    return [c["name"] for c in recipes()]


def case(name):
    return next(c for c in _load()[0]["cases"] if c["name"] == name)


def state(c) -> "OrderedDict[str, np.ndarray]":
    """name -> numpy array (fp32 from the recorded bits, or int64) in the recorded order and shapes."""
    npz = _load()[1]
    out = OrderedDict()
    for key, dtype, shape in c["entries"]:
        a = npz[f"{c['name']}/in/{key}"]
        out[key] = (a.view(np.float32) if dtype == "float32" else a).reshape(tuple(shape))
    return out


def state_dict(c) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, torch.from_numpy(np.array(a))) for k, a in state(c).items())


def wire(c) -> "OrderedDict[str, bytes]":
    """name -> the bytes the reference produced."""
    npz = _load()[1]
    return OrderedDict((key, npz[f"{c['name']}/out/{key}"].tobytes()) for key, _, _ in c["entries"])
