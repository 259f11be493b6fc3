"""Loading and replaying the reference-generated Fl-trust cases (tests/golden/fltrust_*).

A case = recipe (model, K, seed, the slots negated and the slots reduced to their noise) + what the
reference's ``aggregations.fl_trust`` produced: its fp32 scalars (dots, norms, cosines, clipped cosines,
their sum, the normalised weights), SHA-256 of its outputs, the result dtypes, sampled values, full
arrays for two small lenet5 cases, and two float64 error figures per client that bound how far a
correct cosine may sit from the reference's (``ref_self_err``, ``mean_order_shift``).

The inputs are those of ``krum_cases.build_inputs`` with some clients negated (their cosine with the
mean is negative: the ReLU clips them) and some reduced to their noise x - baseline (cosine near 0).
``mirror`` (K = 2) makes row 1 the negation of row 0: the mean is exactly 0, both cosines are 0 and the
output is all +0.  On ResNet-18 the counters are negated with the fp32 entries: they are 99.998 % of
|x|^2, so negating the fp32 entries alone would leave every cosine at 1.
"""

from __future__ import annotations

import json
import os

import numpy as np

from tests import krum_cases as kc
from tests.golden_cases import GOLDEN, canon, hexf, sha  # noqa: F401
from tests.krum_cases import flat_result, sample_index, state_dicts  # noqa: F401

FULL_KS = (8, 33)  # lenet5 cases with full arrays (a committed file stays under 1 MiB)


def recipes():
    def one(model, k, negate=(), noise_only=(), mirror=False):
        return {"name": f"fltrust_{model}_k{k}", "model": model, "k": k, "seed": 700 + k,
                "negate": list(negate), "noise_only": list(noise_only), "mirror": mirror}

    return [one("lenet5", 1), one("lenet5", 2, mirror=True), one("lenet5", 8, (1, 5), (3,)),
            one("lenet5", 33, (0, 7, 20), (4, 9)), one("lenet5", 64, range(0, 64, 5), (3,)),
            one("resnet18", 8, (2, 5), (6,))]


def build_inputs(recipe):
    """(layout, X_f32 [K, n_f32] float32, X_i64 [K, n_i64] int64) of a recipe, in client order."""
    from oracle import synth

    layout, xf, xi = kc.build_inputs(recipe)
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, recipe["seed"])
    for s in recipe["noise_only"]:
        xf[s] = (xf[s] - bf).astype(np.float32)
        xi[s] = xi[s] - bi
    for s in recipe["negate"]:
        xf[s] = -xf[s]
        xi[s] = -xi[s]
    if recipe["mirror"]:
        xf[1] = -xf[0]
        xi[1] = -xi[0]
    return layout, xf, xi


def hexes(values) -> np.ndarray:
    return np.array([hexf(b) for b in values], dtype=np.float32)


def reference_scalars(case) -> dict:
    """The reference's fp32 scalars of a case, in the shape of ``plato_amd.trust.fltrust_weights``."""
    exp = case["expected"]
    return {"nm": hexf(exp["nm"]), "dots": hexes(exp["dots"]), "norms": hexes(exp["norms"]),
            "norms_eps": hexes(exp["norms_eps"]), "div": hexes(exp["norms_eps"]), "cos": hexes(exp["cos"]),
            "clipped": hexes(exp["clipped"]), "weights": hexes(exp["weights"])}


def reference_values(case, full=None):
    return kc.reference_values(case, full)


def load_cases():
    with open(os.path.join(GOLDEN, "fltrust_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    return np.load(os.path.join(GOLDEN, "fltrust_full_small.npz"), allow_pickle=False)
