"""Seeded inputs of the elastic sub-model aggregation tests and fixtures (tests/golden/make_golden_elastic.py
feeds the same inputs to the reference's sysheterofl Algorithm.aggregation).

Two model families, as (name, shape, dtype) lists in state_dict order:

* ``resnet_spec(depths, rates)``: the state_dict of the reference's ``ResnetWrapper(configs=[depths, rates])``
  (examples/model_search/sysheterofl/resnet.py): ``depths[s]`` blocks in stage s at ``ceil(rates[s] * (64, 128,
  256, 512)[s])`` channels.  A client with fewer blocks lacks the keys of the others.  The generator checks
  the list against the reference's own model.
* ``toy_spec(cfg)``: a 3-D ``pos``, a 0-D float ``scale``, a convolution whose kernel the clients cut (5x5
  globally; 3x3, 1x5 and 5x5 clients), a normalisation with its buffers and int64 counter, a 3x3 convolution
  that every client has in full, a 1x1 convolution that one client holds and a head.  The generator builds
  the same module from torch.nn layers.

Values come from tests/submodel_cases.fill, seeded per (case, client, entry).
"""

from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np

from tests import submodel_cases as sc
from tests.submodel_cases import F32, GOLDEN, I64, as_torch, canon, digest, sample_index  # noqa: F401

SPECIAL_BITS = sc.SPECIAL_BITS  # 1e8, -0.0, +inf, NaN, -inf
WIDTHS = (64, 128, 256, 512)

SMALL = ([3, 2, 3, 2], [0.125, 0.125, 0.0625, 0.0625])  # the global model of cases (a) to (c): 8, 16, 16, 32
# (depths, width rate per stage as a multiple of the global's): client 1 has the full configuration; no other
# client holds the third block of stage 1 or 3, or the full width of stage 2
SMALL_CLIENTS = [([2, 2, 2, 2], [0.5, 0.5, 0.5, 0.5]),
                 ([3, 2, 3, 2], [1, 1, 1, 1]),
                 ([2, 2, 2, 2], [1, 0.5, 0.25, 0.5]),
                 ([2, 2, 2, 2], [0.25, 0.25, 0.5, 0.25]),
                 ([2, 2, 2, 2], [0.5, 0.5, 1, 1])]
FULL_CLIENT = 1
# case (b): special values at elements every client covers (the leading ones of COVERED), at elements no
# client covers (its trailing ones: no client there has the full width of stage 2) and in an entry nobody holds
COVERED = "model.layer2.1.conv1.weight"
UNHELD = ("model.layer3.2.conv1.weight", "model.layer1.2.batchnorm1.running_var")

LARGE = ([3, 4, 6, 3], [0.25, 0.25, 0.25, 0.25])  # case (e): ResNet-34 depths at 16, 32, 64, 128 channels

TOY_GLOBAL = dict(c1=7, cin=3, k=(5, 5), cm=5, extra=6, pos=(5, 6, 8))
TOY_CLIENTS = [dict(c1=4, cin=3, k=(3, 3), cm=3, extra=None, pos=(3, 3, 4)),
               dict(c1=7, cin=2, k=(1, 5), cm=5, extra=None, pos=(5, 6, 8)),
               dict(c1=2, cin=3, k=(5, 5), cm=2, extra=3, pos=(1, 1, 1))]


def _bn(prefix, c):
    return sc._bn(prefix, c)


def resnet_spec(depths, rates):
    hidden = [int(np.ceil(r * x)) for r, x in zip(rates, WIDTHS)]  # the reference's own rounding
    spec = [("model.conv1.weight", (hidden[0], 3, 3, 3), F32)]
    inp = hidden[0]
    for layer, (planes, stride, blocks) in enumerate(zip(hidden, (1, 2, 2, 2), depths), start=1):
        for block in range(blocks):
            s = stride if block == 0 else 1
            p = f"model.layer{layer}.{block}"
            spec += _bn(p + ".batchnorm1", inp)
            spec.append((p + ".conv1.weight", (planes, inp, 3, 3), F32))
            spec += _bn(p + ".batchnorm2", planes)
            spec.append((p + ".conv2.weight", (planes, planes, 3, 3), F32))
            if s != 1 or inp != planes:
                spec.append((p + ".shortcut.weight", (planes, inp, 1, 1), F32))
            inp = planes
    spec += _bn("model.bn4", hidden[3])
    spec += [("model.linear.weight", (10, hidden[3]), F32), ("model.linear.bias", (10,), F32)]
    return spec


def toy_spec(cfg):
    c1, cm = cfg["c1"], cfg["cm"]
    spec = [("pos", tuple(cfg["pos"]), F32), ("scale", (), F32),
            ("conv.weight", (c1, cfg["cin"], *cfg["k"]), F32), ("conv.bias", (c1,), F32)]
    spec += _bn("norm", c1)
    spec.append(("mix.weight", (cm, c1, 3, 3), F32))
    if cfg["extra"]:
        spec += [("extra.weight", (cfg["extra"], cm, 1, 1), F32), ("extra.bias", (cfg["extra"],), F32)]
    spec += [("head.weight", (10, cm), F32), ("head.bias", (10,), F32)]
    return spec


def _scaled(config, mult):
    return [list(mult[0]), [g * m for g, m in zip(config[1], mult[1])]]


def large_clients(seed: int, k: int = 7):
    """Seeded (depths, rates) of case (e): each stage's depth in 2..max, its width the global's times 1, 1/2 or 1/4."""
    rng = np.random.default_rng([seed, 77])
    return [[[int(rng.integers(2, d + 1)) for d in LARGE[0]],
             [r * float(rng.choice([1.0, 0.5, 0.25])) for r in LARGE[1]]] for _ in range(k)]


def recipes():
    small = [_scaled(SMALL, c) for c in SMALL_CLIENTS]
    partial = [c for i, c in enumerate(small) if i != FULL_CLIENT]
    return [
        dict(name="resnet_small", model="resnet", config=[list(SMALL[0]), list(SMALL[1])], clients=small, seed=201,
             update_track=True, special=False, full=True, unheld=False),
        dict(name="resnet_small_partial", model="resnet", config=[list(SMALL[0]), list(SMALL[1])], clients=partial,
             seed=202, update_track=True, special=True, full=True, unheld=True),
        dict(name="resnet_small_no_track", model="resnet", config=[list(SMALL[0]), list(SMALL[1])], clients=small,
             seed=201, update_track=False, special=False, full=True, unheld=False),
        dict(name="toy", model="toy", config=TOY_GLOBAL, clients=TOY_CLIENTS, seed=204, update_track=True,
             special=False, full=True, unheld=False),
        dict(name="resnet34_quarter", model="resnet", config=[list(LARGE[0]), list(LARGE[1])],
             clients=large_clients(205), seed=205, update_track=True, special=False, full=False, unheld=None),
    ]


def spec_of(model: str, config):
    return resnet_spec(*config) if model == "resnet" else toy_spec(config)


def special_positions(g):
    """[(entry, flat index, bits)] of case (b): every special value at an element all clients cover, at one
    no client covers, and in two entries that nobody holds (one of them a running statistic)."""
    n = g[COVERED].size
    out = [(COVERED, h, b) for h, b in enumerate(SPECIAL_BITS)]
    out += [(COVERED, n - 1 - h, b) for h, b in enumerate(SPECIAL_BITS)]
    for name in UNHELD:
        out += [(name, h, b) for h, b in enumerate(SPECIAL_BITS)]
    return out


def build(recipe):
    """(global model, clients) as name -> ndarray dicts; a client holds the keys of its own configuration."""
    g = sc.fill(spec_of(recipe["model"], recipe["config"]), recipe["seed"], 0)
    if recipe["special"]:
        for name, at, bits in special_positions(g):
            g[name].reshape(-1).view(np.uint32)[at] = bits
    clients = [sc.fill(spec_of(recipe["model"], c), recipe["seed"], 1 + k) for k, c in enumerate(recipe["clients"])]
    return g, clients


def all_flat(result) -> np.ndarray:
    """Every entry of a result (all float32), canonicalised, in key order."""
    parts = [canon(np.asarray(a)).reshape(-1) for a in result.values()]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def load_cases():
    with open(os.path.join(GOLDEN, "elastic_cases.json")) as f:
        return json.load(f)["cases"]


def load_full(name: str):
    with np.load(os.path.join(GOLDEN, f"elastic_full_{name}.npz")) as z:
        return OrderedDict((k, z[k]) for k in z.files)
