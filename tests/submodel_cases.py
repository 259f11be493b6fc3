"""Seeded inputs of the sub-model aggregation tests and fixtures (tests/golden/make_golden_submodel.py
feeds the same inputs to the reference's Algorithm.aggregation).

Two model families, as (name, shape, dtype) lists in state_dict order:

* ``resnet18_spec``: the state_dict of the reference's HeteroFL ResNet-18
  (examples/model_search/heterofl/resnet.py, ``track=True``) at hidden sizes ``ceil(rate * (64, 128,
  256, 512))``.  The generator checks the list against the reference's own model.
* ``toy_spec``: a 3-D ``pos_weight``, a 0-D ``s_bias``, a convolution with 3 input channels (27-float
  rows), a normalisation with its buffers and int64 counter, a 1x1 convolution and a head whose dim 0
  is full at every rate.  The generator builds the same module from torch.nn layers.

Values are ``standard_normal`` scaled to the order of trained weights, seeded per (case, client, entry).
"""

from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
F32, I64 = "float32", "int64"
SCALE = 0.05
RATES_FULL = (0.5, 0.0625, 0.25, 0.125, 0.5, 0.25, 0.0625)   # case (b): the seven clients of the full ResNet-18
SPECIAL_BITS = (0x4CBEBC20, 0x80000000, 0x7F800000, 0x7FC00000, 0xFF800000)  # 1e8, -0.0, +inf, NaN, -inf
SPECIAL_ENTRY = "layer1.0.conv1.weight"
TOY_FULL = (7, 13, (5, 6, 8))  # stem channels, mixed channels, pos_weight


def ceil_rate(rate: float, x: int) -> int:
    return int(np.ceil(rate * x))  # the reference's own rounding (resnet.py: hidden_size)


def _bn(prefix, c):
    return [(prefix + ".weight", (c,), F32), (prefix + ".bias", (c,), F32), (prefix + ".running_mean", (c,), F32),
            (prefix + ".running_var", (c,), F32), (prefix + ".num_batches_tracked", (), I64)]


def resnet18_spec(rate: float):
    hidden = [ceil_rate(rate, x) for x in (64, 128, 256, 512)]
    spec = [("conv1.weight", (hidden[0], 3, 3, 3), F32)]
    inp = hidden[0]
    for layer, (planes, stride) in enumerate(zip(hidden, (1, 2, 2, 2)), start=1):
        for block, s in enumerate((stride, 1)):
            p = f"layer{layer}.{block}"
            spec += _bn(p + ".batchnorm1", inp)
            spec.append((p + ".conv1.weight", (planes, inp, 3, 3), F32))
            spec += _bn(p + ".batchnorm2", planes)
            spec.append((p + ".conv2.weight", (planes, planes, 3, 3), F32))
            if s != 1 or inp != planes:
                spec.append((p + ".shortcut.weight", (planes, inp, 1, 1), F32))
            inp = planes
    spec += _bn("bn4", hidden[3])
    spec += [("linear.weight", (10, hidden[3]), F32), ("linear.bias", (10,), F32)]
    return spec


def toy_widths(rate: float, full=TOY_FULL):
    c1, c2, pos = full
    return ceil_rate(rate, c1), ceil_rate(rate, c2), tuple(ceil_rate(rate, d) for d in pos)


def toy_spec(rate: float, full=TOY_FULL):
    c1, c2, pos = toy_widths(rate, full)
    return ([("pos_weight", pos, F32), ("s_bias", (), F32), ("stem.weight", (c1, 3, 3, 3), F32)] + _bn("norm", c1)
            + [("mix.weight", (c2, c1, 1, 1), F32), ("mix.bias", (c2,), F32),
               ("head.weight", (10, c2), F32), ("head.bias", (10,), F32)])


def spec_of(model: str, rate: float):
    return resnet18_spec(rate) if model == "resnet18" else toy_spec(rate)


def recipes():
    small = 0.0625
    toy_rates = [0.5, 0.125, 0.25, 1.0, 0.5]
    out = [
        # (a) the smallest ResNet-18 as the global model, its clients at that rate times 1, 1/2, 1/4, 1/8
        dict(name="resnet18_small", model="resnet18", algo="heterofl", global_rate=small,
             client_rates=[small * m for m in (0.5, 1.0, 0.25, 0.125, 0.5, 0.25)], seed=101, full=True),
        # the same without the full-width client: elements no client covers
        dict(name="resnet18_small_partial", model="resnet18", algo="fedrolex", global_rate=small,
             client_rates=[small * m for m in (0.5, 0.125, 0.25, 0.5, 0.125, 0.25)], seed=102, full=True),
        dict(name="resnet18_small_special", model="resnet18", algo="heterofl", global_rate=small,
             client_rates=[small * m for m in (0.25, 0.5, 0.125, 0.5)], seed=103, full=True, special=True),
        # (b) the full ResNet-18
        dict(name="resnet18_full", model="resnet18", algo="heterofl", global_rate=1.0,
             client_rates=list(RATES_FULL), seed=104, full=False),
        dict(name="resnet18_full_rolex", model="resnet18", algo="anycostfl", global_rate=1.0,
             client_rates=list(RATES_FULL[::-1]), seed=105, full=False),
    ]
    # (c) the toy module under the four reference classes: the two rules differ on the 3-D entry
    for i, algo in enumerate(("heterofl", "fjord", "fedrolex", "anycostfl")):
        out.append(dict(name=f"toy_{algo}", model="toy", algo=algo, global_rate=1.0, client_rates=toy_rates,
                        seed=110 + i, full=True))
    for r in out:
        r["rule"] = RULE_OF[r["algo"]]
        r.setdefault("special", False)
    return out


RULE_OF = {"heterofl": "heterofl", "fjord": "heterofl", "fedrolex": "fedrolex", "anycostfl": "fedrolex"}


def fill(spec, seed: int, who: int):
    """name -> ndarray for one model: ``who`` 0 is the global model, 1 + k client k."""
    out = OrderedDict()
    for idx, (name, shape, dtype) in enumerate(spec):
        rng = np.random.default_rng([seed, who, idx])
        if dtype == I64:
            out[name] = rng.integers(0, 1000, size=shape, dtype=np.int64)
        elif name.endswith("running_var"):
            out[name] = (1.0 + SCALE * rng.standard_normal(shape)).astype(np.float32)
        else:
            out[name] = (SCALE * rng.standard_normal(shape)).astype(np.float32)
    return out


def special_positions(numel: int):
    """[(flat index, bits)] in SPECIAL_ENTRY: the leading elements (every client covers them) and the
    trailing ones (no client below full width covers them) take each special value."""
    return [(h, b) for h, b in enumerate(SPECIAL_BITS)] + [(numel - 1 - h, b) for h, b in enumerate(SPECIAL_BITS)]


def build(recipe):
    """(global model, clients) as name -> ndarray dicts."""
    g = fill(spec_of(recipe["model"], recipe["global_rate"]), recipe["seed"], 0)
    if recipe.get("special"):
        flat = g[SPECIAL_ENTRY].reshape(-1).view(np.uint32)
        for at, b in special_positions(flat.size):
            flat[at] = b
    clients = [fill(spec_of(recipe["model"], rate), recipe["seed"], 1 + k)
               for k, rate in enumerate(recipe["client_rates"])]
    return g, clients


def as_torch(model):
    import torch

    return OrderedDict((name, torch.from_numpy(np.array(a))) for name, a in model.items())


# ------------------------------------------------------------------ fixtures
CANON_NAN = np.uint32(0x7FC00000)


def canon(a: np.ndarray) -> np.ndarray:
    """float32 with every NaN as one bit pattern (tests/golden/make_golden.canon); other dtypes as they are."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    a = a.copy()
    a.reshape(-1).view(np.uint32)[np.isnan(a.reshape(-1))] = CANON_NAN
    return a


def digest(result) -> str:
    """SHA-256 over the canonicalised entries' bytes, in key order."""
    import hashlib

    h = hashlib.sha256()
    for name, a in result.items():
        h.update(name.encode())
        h.update(canon(np.asarray(a)).tobytes())
    return h.hexdigest()


def sample_index(n: int, count: int = 64):
    return np.unique(np.linspace(0, n - 1, num=min(count, n), dtype=np.int64)) if n else np.zeros(0, dtype=np.int64)


def participating_flat(result) -> np.ndarray:
    parts = [canon(np.asarray(a)).reshape(-1) for name, a in result.items() if "weight" in name or "bias" in name]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def load_cases():
    with open(os.path.join(GOLDEN, "submodel_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    with np.load(os.path.join(GOLDEN, "submodel_full_small.npz")) as z:
        return {k: z[k] for k in z.files}
