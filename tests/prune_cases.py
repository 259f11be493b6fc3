"""The seeded pruning models and their reference-generated fixtures (tests/golden/prune_cases.json, .npz).

A case is one model, its state as raw bits, an ``amount`` and a number of successive applications of the
reference's ``unstructured_pruning`` processor; the fixture keeps the state after every application (raw
bits, nothing canonicalised) and the key order of ``state_dict()``.  The generator
(tests/golden/make_golden_prune.py) asserts for every application that the reference's answer is the only
possible one, so every comparison is bit for bit.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON_PATH = os.path.join(GOLDEN, "prune_cases.json")
NPZ_PATH = os.path.join(GOLDEN, "prune_full_small.npz")


class _Block(torch.nn.Module):
    """A narrow ResNet basic block with a projection shortcut (convolutions without bias)."""

    def __init__(self, cin=3, cout=5):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, stride=2, padding=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(cout)
        self.conv2 = torch.nn.Conv2d(cout, cout, 3, padding=1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(cout)
        self.shortcut = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=2, bias=False),
                                            torch.nn.BatchNorm2d(cout))


class _ResNetBlock(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 3, 3, padding=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(3)
        self.layer1 = _Block(3, 5)
        self.linear = torch.nn.Linear(5, 7)


def build(model: str) -> torch.nn.Module:
    """The module tree of a fixture model (the weights come from the fixture)."""
    nn = torch.nn
    if model == "toy":  # conv + batch-norm + linear
        return nn.Sequential(nn.Conv2d(2, 4, 3), nn.BatchNorm2d(4), nn.ReLU(), nn.Flatten(), nn.Linear(36, 5))
    if model == "lenet5":
        return nn.Sequential(nn.Conv2d(1, 6, 5), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(6, 16, 5), nn.ReLU(),
                             nn.MaxPool2d(2), nn.Flatten(), nn.Linear(400, 120), nn.ReLU(), nn.Linear(120, 84),
                             nn.ReLU(), nn.Linear(84, 10))
    if model == "resblock":
        return _ResNetBlock()
    raise KeyError(model)


def recipes():
    """name, model, seed, amount, applications, edits.  An edit names what the generator writes into the
    prunable weights before the first application (make_golden_prune.py: EDITS)."""
    def one(name, model, seed, amount, applications=1, edit=None):
        return {"name": name, "model": model, "seed": seed, "amount": amount, "applications": applications,
                "edit": edit}

    # the toy model has n = 252 prunable weights: 0.125 n = 31.5 -> 32 and 0.375 n = 94.5 -> 94
    return [
        one("toy_float", "toy", 5101, 0.2),
        one("toy_int", "toy", 5102, 37),
        one("toy_half_up", "toy", 5103, 0.125),
        one("toy_half_down", "toy", 5104, 0.375),
        one("toy_zero_int", "toy", 5105, 0),
        one("toy_zero_float", "toy", 5106, 0.0),
        one("toy_all_float", "toy", 5107, 1.0),
        one("toy_all_int", "toy", 5108, 252),
        one("toy_thrice", "toy", 5109, 0.3, applications=3),
        one("toy_many_zeros", "toy", 5110, 0.2, edit="zeros"),
        one("toy_nonfinite_kept", "toy", 5111, 0.2, edit="nonfinite"),
        one("toy_nonfinite_all", "toy", 5112, 1.0, edit="nonfinite_snan"),
        one("toy_inf_pruned_nan_kept", "toy", 5113, 249, edit="nonfinite"),
        one("toy_nonfinite_twice", "toy", 5114, 250, applications=2, edit="nonfinite"),
        one("toy_subnormals", "toy", 5115, 26, edit="subnormals"),
        one("resblock_half", "resblock", 5116, 0.5, applications=2),
        one("lenet5_most", "lenet5", 5117, 0.8),
    ]


@functools.lru_cache(maxsize=None)
def _load():
    with open(JSON_PATH) as f:
        meta = json.load(f)
    return meta, np.load(NPZ_PATH)


def cases():
    return _load()[0]["cases"]


def case_ids():
    return [c["name"] for c in recipes()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def amount_of(c):
    return int(c["amount"]) if c["amount_type"] == "int" else float(c["amount"])


def state_bits(c, stage: str):
    """``stage`` is "in" or "out<a>" (a = 1.. applications): name -> raw bits (uint32 for fp32 entries, int64
    for counters), in the recorded ``state_dict()`` order of that stage."""
    npz = _load()[1]
    keys = c["keys_in"] if stage == "in" else c["keys_out"][int(stage[3:]) - 1]
    return {k: npz[f"{c['name']}/{stage}/{k}"] for k in keys}


def load_model(c, stage: str = "in") -> torch.nn.Module:
    model = build(c["model"])
    bits = state_bits(c, stage)
    with torch.no_grad():
        for k, t in model.state_dict().items():
            a = bits[k]
            src = torch.from_numpy(a.view(np.float32) if a.dtype == np.uint32 else a).reshape(t.shape)
            t.copy_(src)
    return model


def model_bits(model) -> dict:
    """``state_dict()`` of a module as raw bits, in its order."""
    out = {}
    for k, t in model.state_dict().items():
        a = t.detach().cpu().contiguous().numpy().reshape(-1)
        out[k] = a.view(np.uint32).copy() if a.dtype == np.float32 else a.astype(np.int64)
    return out


def prunable_names(model) -> list[str]:
    """The state-dict names of the prunable weights, in the reference's order."""
    return [f"{name}.weight" if name else "weight" for name, m in model.named_modules()
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))]


def as_row(bits: dict, prunable: list[str]):
    """Every entry of a state as one row of 32-bit words in ``bits``' order (an int64 counter is two words),
    and the pieces of the prunable entries in ``prunable`` order.  The state-dict order of the fixture models
    keeps the prunable weights ascending."""
    words, where, at = [], {}, 0
    for k, a in bits.items():
        w = a.view(np.uint32).reshape(-1)
        where[k] = (at, at + w.size)
        words.append(w)
        at += w.size
    return np.concatenate(words), [where[k] for k in prunable], where
