"""Loading and replaying the reference-generated Bulyan and Trimmed-mean cases (tests/golden/bulyan_*).

A case = recipe (kind, model, K, seed, f) + what the reference's ``aggregations.bulyan`` or
``aggregations.trimmed_mean`` produced: its selection order (Bulyan), SHA-256 of its fp32 and
int64-as-fp32 outputs, the result dtypes, sampled values, and full arrays for the small lenet5 cases.
The inputs are ``krum_cases.build_inputs``' construction (scaled noise, a seeded permutation), shared
with the generator (tests/golden/make_golden_bulyan.py).

``recipe["tie_f32"]`` / ``recipe["tie_i64"]`` list the boundary-tie columns of the coordinate-wise
step (nearest_oracle.boundary_tie_columns): there the reference may keep another of the equally distant
values than the table-order rule does, and a result is compared with the restatement instead.
"""

from __future__ import annotations

import json
import os

import numpy as np

from tests import krum_cases as kc  # noqa: F401
from tests import nearest_oracle as no
from tests.golden_cases import GOLDEN, canon, hexf, sha  # noqa: F401
from tests.krum_cases import build_inputs, flat_result, reference_values, sample_index, state_dicts  # noqa: F401

BULYAN_LENET = ((13, 3), (16, 3), (33, 3), (64, 5), (9, 2), (6, 1))  # (K, f)
# ResNet-18 (int64 counters among the entries) at (6, 1), not at (13, 3): the generator's separation
# condition at that size (relative gap >= 0.05 at every step, make_golden_krum.py) cannot be met at
# (13, 3) with build_inputs' noise scales (1 + c/8).  At the step with m = 8 remaining clients the expected
# gap is 0.035, and the best of 20,000 seeds reaches 0.0494 (seed 10010, m = 8; make_golden_bulyan.py
# --search resnet18:13:3:513:20513).  Bulyan on ResNet-18 at (13, 3) is checked on the GPU against the
# restatement instead (tests/test_bulyan_gpu.py, RESNET_13_3).
BULYAN_RESNET = ((6, 1),)
TRIMMED_LENET = (1, 2, 8, 33)
TRIMMED_RESNET = (8,)
FULL = ("bulyan_lenet5_k13_f3", "bulyan_lenet5_k6_f1", "trimmed_lenet5_k8")  # a committed file stays under 1 MiB
MAX_TIES_LENET = 8


def trim_of(recipe) -> int:
    """``trim`` of the coordinate-wise step: f for Bulyan, the reference's hard-coded 0 for Trimmed-mean."""
    return recipe["f"] if recipe["kind"] == "Bulyan" else 0


def tie_columns(recipe, xf, xi, selection):
    """(fp32 region, int64 region) boundary-tie columns of the case's coordinate-wise step."""
    rows = list(selection) if recipe["kind"] == "Bulyan" else list(range(xf.shape[0]))
    t = trim_of(recipe)
    tf = no.boundary_tie_columns(xf[rows], t)
    ti = no.boundary_tie_columns(xi[rows], t) if xi.size else np.zeros(0, dtype=np.int64)
    return tf, ti


def load_cases():
    with open(os.path.join(GOLDEN, "bulyan_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    return np.load(os.path.join(GOLDEN, "bulyan_full_small.npz"), allow_pickle=False)
