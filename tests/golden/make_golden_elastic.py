"""Generate the elastic sub-model aggregation fixtures from the reference (TL-System/plato,
examples/model_search/sysheterofl).

    python tests/golden/make_golden_elastic.py --reference /path/to/plato

Runs ``Algorithm.aggregation`` of sysheterofl_algorithm.py on the inputs of tests/elastic_cases.build and writes

    tests/golden/elastic_cases.json          recipe, SHA-256 of the canonicalised outputs, dtypes, samples,
                                             coverage counts, the entries nobody holds
    tests/golden/elastic_full_<case>.npz     full outputs of the cases stored in full, by key

``aggregation()`` reads ``self.model`` only: the instance is made with ``Algorithm.__new__`` and given its
model.  For the ResNet cases the model is the reference's own ``ResnetWrapper(configs=...)`` with the seeded
values loaded, and every client is built by the same class at its configuration (its keys and shapes are
checked against tests/elastic_cases); for the toy case it is the module below.  Per case the generator
asserts that there are elements covered by every client, by some and by none, an entry that no client holds
where the case has one, that every result is float32, that the reference leaves ``(g - g) / 1`` where nobody
reaches and that it leaves its model unchanged; in the special-value case 1e8, -0.0, +-inf and NaN sit at
covered positions, at uncovered ones and in entries nobody holds.
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

from tests import elastic_cases as ec  # noqa: E402
from tests import elastic_oracle as eo  # noqa: E402


def toy_module(cfg):
    import torch
    from torch import nn

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.pos = nn.Parameter(torch.zeros(cfg["pos"]))
            self.scale = nn.Parameter(torch.zeros(()))
            self.conv = nn.Conv2d(cfg["cin"], cfg["c1"], tuple(cfg["k"]))
            self.norm = nn.BatchNorm2d(cfg["c1"])
            self.mix = nn.Conv2d(cfg["c1"], cfg["cm"], 3, bias=False)
            if cfg["extra"]:
                self.extra = nn.Conv2d(cfg["cm"], cfg["extra"], 1)
            self.head = nn.Linear(cfg["cm"], 10)

    return Toy()


def check_spec(model, spec, what):
    got = [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in model.state_dict().items()]
    assert got == [(n, tuple(s), d) for n, s, d in spec], (what, got[:4], spec[:4])


def coverage(counts, k):
    none = sum(int((c == 0).sum()) for c in counts.values())
    every = sum(int((c == k).sum()) for c in counts.values())
    some = sum(int(((c > 0) & (c < k)).sum()) for c in counts.values())
    return {"none": none, "all": every, "some": some}


def run_case(recipe, algorithm, wrapper):
    import torch

    g, clients = ec.build(recipe)
    if recipe["model"] == "resnet":
        make = lambda config: wrapper(configs=config)  # noqa: E731
    else:
        make = toy_module
    model = make(recipe["config"])
    check_spec(model, ec.spec_of(recipe["model"], recipe["config"]), recipe["name"])
    model.load_state_dict(ec.as_torch(g))
    for config in recipe["clients"]:
        check_spec(make(config), ec.spec_of(recipe["model"], config), (recipe["name"], config))
    algo = algorithm.Algorithm.__new__(algorithm.Algorithm)
    algo.model = model
    before = OrderedDict((k, v.clone()) for k, v in model.state_dict().items())
    with torch.no_grad():
        result = algo.aggregation([ec.as_torch(c) for c in clients], update_track=recipe["update_track"])
    assert list(result) == list(g)
    for k, v in model.state_dict().items():  # the reference leaves its model alone
        assert v.dtype == before[k].dtype and v.numpy().tobytes() == before[k].numpy().tobytes()
    assert all(v.dtype == torch.float32 for v in result.values())
    out = OrderedDict((k, v.detach().numpy().copy()) for k, v in result.items())

    _, counts = eo.aggregate(g, clients, recipe["update_track"])
    cov = coverage(counts, len(clients))
    assert cov["all"] > 0 and cov["some"] > 0 and cov["none"] > 0, (recipe["name"], cov)
    unheld = [k for k in g if g[k].dtype == np.float32 and eo.rank_of(k, g[k].ndim, recipe["update_track"])
              and not any(k in c for c in clients)]
    if recipe["unheld"] is not None:  # an entry that no client holds, where the case is built to have one
        assert bool(unheld) == recipe["unheld"], (recipe["name"], unheld)
    for name, c in counts.items():  # where no client reaches, the reference gives (g - g) / 1
        dead = c == 0
        with np.errstate(invalid="ignore"):
            want = (g[name] - g[name]).astype(np.float32)[dead]
        assert np.array_equal(ec.canon(out[name][dead]).view(np.uint32), ec.canon(want).view(np.uint32)), name
    if recipe["special"]:
        n = len(ec.SPECIAL_BITS)
        pos = ec.special_positions(g)
        cnt = [int(counts[name].reshape(-1)[at]) for name, at, _ in pos]
        assert cnt[:n] == [len(clients)] * n and not any(cnt[n:]), cnt
        assert all(name in unheld for name in ec.UNHELD)

    flat = ec.all_flat(out)
    idx = ec.sample_index(flat.size)
    if recipe["full"]:
        np.savez_compressed(os.path.join(HERE, f"elastic_full_{recipe['name']}.npz"),
                            **{k: ec.canon(v) for k, v in out.items()})
    return {"recipe": recipe,
            "expected": {"sha": ec.digest(out), "dtypes": {k: str(v.dtype) for k, v in out.items()},
                         "coverage": cov, "unheld": unheld, "n_elements": int(flat.size),
                         "samples": [[int(j), "%08x" % int(flat.view(np.uint32)[j])] for j in idx]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    make_golden.STUBBED.append("ptflops")  # not installed; aggregation() never calls it
    with tempfile.TemporaryDirectory() as work:
        boot_reference(args.reference, work)
        here = os.path.join(args.reference, "examples/model_search/sysheterofl")
        sys.path.insert(0, here)
        algorithm = __import__("sysheterofl_algorithm")
        spec = importlib.util.spec_from_file_location("sysheterofl_resnet", os.path.join(here, "resnet.py"))
        resnet = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(resnet)

        cases = []
        for recipe in ec.recipes():
            cases.append(run_case(recipe, algorithm, resnet.ResnetWrapper))
            print(recipe["name"], cases[-1]["expected"]["coverage"], len(cases[-1]["expected"]["unheld"]), flush=True)
    with open(os.path.join(HERE, "elastic_cases.json"), "w") as f:
        json.dump({"reference": "examples/model_search/sysheterofl: Algorithm.aggregation", "cases": cases}, f, indent=0)


if __name__ == "__main__":
    main()
