"""Generate the sub-model aggregation fixtures from the reference (TL-System/plato, examples/model_search).

    python tests/golden/make_golden_submodel.py --reference /path/to/plato

Runs ``Algorithm.aggregation`` of heterofl_algorithm.py, fjord_algorithm.py, fedrolex_algorithm.py and
anycostfl_algorithm.py on the inputs of tests/submodel_cases.build and writes

    tests/golden/submodel_cases.json        recipe, SHA-256 of the canonicalised outputs, dtypes, samples,
                                            coverage counts
    tests/golden/submodel_full_small.npz    full outputs of the small cases ("<case>|<key>")

``aggregation()`` reads ``self.model`` only.  For the ResNet-18 cases the model is the reference's own
HeteroFL ``resnet18(model_rate, track=True)`` with the seeded values loaded, and every client is built by
the same class at its rate (its shapes are checked against tests/submodel_cases); for the toy cases it is
the module below.  Per case the generator asserts that the output has an element covered by every client,
one covered by some, and (unless a client has the full width and every entry has a rank) one covered by
none; in the special-value case 1e8, -0.0, +-inf and NaN sit at covered and at uncovered positions.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import tempfile
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from make_golden import boot_reference  # noqa: E402

from tests import submodel_cases as sc  # noqa: E402
from tests import submodel_oracle as so  # noqa: E402

ALGOS = ("heterofl", "fjord", "fedrolex", "anycostfl")


def toy_module(rate):
    import torch
    from torch import nn

    c1, c2, pos = sc.toy_widths(rate)

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.pos_weight = nn.Parameter(torch.zeros(pos))
            self.s_bias = nn.Parameter(torch.zeros(()))
            self.stem = nn.Conv2d(3, c1, 3, bias=False)
            self.norm = nn.BatchNorm2d(c1)
            self.mix = nn.Conv2d(c1, c2, 1)
            self.head = nn.Linear(c2, 10)

    return Toy()


def check_spec(model, spec, what):
    got = [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in model.state_dict().items()]
    assert got == [(n, tuple(s), d) for n, s, d in spec], (what, got[:4], spec[:4])


def coverage(counts, k):
    none = sum(int((c == 0).sum()) for c in counts.values())
    every = sum(int((c == k).sum()) for c in counts.values())
    some = sum(int(((c > 0) & (c < k)).sum()) for c in counts.values())
    return {"none": none, "all": every, "some": some}


def run_case(recipe, algorithms, resnet18, full):
    import torch

    g, clients = sc.build(recipe)
    if recipe["model"] == "resnet18":
        make = lambda rate: resnet18(model_rate=rate, track=True)  # noqa: E731
    else:
        make = toy_module
    model = make(recipe["global_rate"])
    check_spec(model, sc.spec_of(recipe["model"], recipe["global_rate"]), recipe["name"])
    model.load_state_dict(sc.as_torch(g))
    for rate in recipe["client_rates"]:
        check_spec(make(rate), sc.spec_of(recipe["model"], rate), (recipe["name"], rate))
    algo = algorithms[recipe["algo"]].Algorithm.__new__(algorithms[recipe["algo"]].Algorithm)
    algo.model = model
    before = OrderedDict((k, v.clone()) for k, v in model.state_dict().items())
    with torch.no_grad():
        result = algo.aggregation([sc.as_torch(c) for c in clients])
    assert list(result) == list(g)
    for k, v in model.state_dict().items():  # the reference leaves its model alone
        assert v.dtype == before[k].dtype and v.numpy().tobytes() == before[k].numpy().tobytes()
    out = OrderedDict((k, v.detach().numpy().copy()) for k, v in result.items())

    _, counts = so.aggregate(g, clients, recipe["rule"])
    cov = coverage(counts, len(clients))
    assert cov["all"] > 0 and cov["some"] > 0, (recipe["name"], cov)
    everything_covered = (max(recipe["client_rates"]) >= recipe["global_rate"]
                          and all(so.rank_of(recipe["rule"], c.ndim) for c in counts.values()))
    assert (cov["none"] == 0) == everything_covered, (recipe["name"], cov)
    for name, c in counts.items():  # where no client reaches, the reference gives (g - g) / 1
        dead = c == 0
        with np.errstate(invalid="ignore"):
            want = (g[name] - g[name])[dead]
        assert np.array_equal(sc.canon(out[name][dead]).view(np.uint32), sc.canon(want).view(np.uint32)), name
    if recipe["special"]:
        flat_out = sc.canon(out[sc.SPECIAL_ENTRY]).reshape(-1)
        flat_cnt = counts[sc.SPECIAL_ENTRY].reshape(-1)
        n = len(sc.SPECIAL_BITS)
        pos = sc.special_positions(flat_out.size)
        assert all(flat_cnt[at] == len(clients) for at, _ in pos[:n]) and all(flat_cnt[at] == 0 for at, _ in pos[n:])

    flat = sc.participating_flat(out)
    idx = sc.sample_index(flat.size)
    if recipe["full"]:
        for k, v in out.items():
            full[recipe["name"] + "|" + k] = sc.canon(v)
    return {"recipe": recipe,
            "expected": {"sha": sc.digest(out), "dtypes": {k: str(v.dtype) for k, v in out.items()},
                         "coverage": cov, "n_participating": int(flat.size),
                         "samples": [[int(j), "%08x" % int(flat.view(np.uint32)[j])] for j in idx]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    make_golden.STUBBED.append("ptflops")  # not installed; aggregation() never calls it
    with tempfile.TemporaryDirectory() as work:
        boot_reference(args.reference, work)
        algorithms = {}
        for name in ALGOS:
            sys.path.insert(0, os.path.join(args.reference, "examples/model_search", name))
            algorithms[name] = __import__(name + "_algorithm")
        spec = importlib.util.spec_from_file_location(
            "heterofl_resnet", os.path.join(args.reference, "examples/model_search/heterofl/resnet.py"))
        resnet = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(resnet)

        full, cases = {}, []
        for recipe in sc.recipes():
            cases.append(run_case(recipe, algorithms, resnet.resnet18, full))
            print(recipe["name"], recipe["algo"], cases[-1]["expected"]["coverage"], flush=True)
    with open(os.path.join(HERE, "submodel_cases.json"), "w") as f:
        json.dump({"reference": "examples/model_search/{heterofl,fjord,fedrolex,anycostfl}: Algorithm.aggregation",
                   "cases": cases}, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "submodel_full_small.npz"), **full)


if __name__ == "__main__":
    main()
