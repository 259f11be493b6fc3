"""Loading and replaying the reference-generated Multi-Krum cases (tests/golden/krum_*).

A case = recipe (model, K, seed, f) + what the reference's ``aggregations.multi_krum`` produced: its
selection order, SHA-256 of its fp32 and int64-as-fp32 outputs, the result dtypes, sampled values,
and full arrays for two small lenet5 cases.  The inputs are rebuilt from ``oracle.synth`` by
:func:`build_inputs`, shared with the generator (tests/golden/make_golden_krum.py).

Client c of the generator stream is the baseline plus its noise scaled by (1 + c/8), so the scores
are well separated; the clients are then shuffled by a seeded permutation, so the selection is not
the identity order.  The generator asserts the separation at every selection step.
"""

from __future__ import annotations

import json
import os

import numpy as np

from tests.golden_cases import GOLDEN, canon, hexf, model_spec, sha  # noqa: F401

KS_LENET = (7, 8, 9, 16, 33, 64)
FULL_KS = (7, 16)  # lenet5 cases with full arrays (a committed file stays under 1 MiB)
N_SAMPLES = 64
F = 2  # the reference's hard-coded num_attackers_selected


def permutation(k: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).permutation(k)


def build_inputs(recipe):
    """(layout, X_f32 [K, n_f32] float32, X_i64 [K, n_i64] int64) of a recipe, in client order."""
    from oracle import synth
    from plato_amd.arena import ArenaLayout

    layout = ArenaLayout.from_shapes(model_spec(recipe["model"]))
    k, seed = recipe["k"], recipe["seed"]
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, seed)
    xf = np.empty((k, layout.n_f32), dtype=np.float32)
    xi = np.empty((k, layout.n_i64), dtype=np.int64)
    for slot, c in enumerate(permutation(k, seed)):
        noise = synth.synth_f32(layout.n_f32, seed, int(c) + 1, synth.CLIENT_SCALE)
        scaled = (noise * np.float32(1.0 + int(c) / 8.0)).astype(np.float32)
        xf[slot] = (bf + scaled).astype(np.float32)
        xi[slot] = synth.synth_i64(layout.n_i64, seed, int(c) + 1, synth.I64_CLIENT_MOD, add=bi)
    return layout, xf, xi


def state_dicts(layout, xf, xi):
    import torch

    return [layout.unpack(torch.from_numpy(xf[c]), torch.from_numpy(xi[c])) for c in range(xf.shape[0])]


def sample_index(n: int) -> np.ndarray:
    return np.unique(np.concatenate([np.arange(min(n, 8)), np.linspace(0, n - 1, N_SAMPLES - 8).astype(np.int64)])
                     ) if n else np.zeros(0, dtype=np.int64)


def flat_result(layout, result):
    """(fp32 region, int64 region) of a result dict as float32 arrays, plus the dtypes met."""
    f = [np.asarray(result[e.name].reshape(-1).numpy()) for e in layout.entries if e.region == "f32"]
    i = [np.asarray(result[e.name].reshape(-1).numpy()) for e in layout.entries if e.region == "i64"]
    dtypes = sorted({str(result[e.name].dtype) for e in layout.entries})
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)  # noqa: E731
    return cat(f), cat(i), dtypes


def reference_values(case, full=None):
    """[(region, indices, reference values)] a result is compared against: the sampled values, and the
    whole fp32 region where the fixture stores it."""
    exp, name = case["expected"], case["recipe"]["name"]
    out = []
    for region, key in (("f32", "samples_f32"), ("i64", "samples_i64f")):
        if exp[key]:
            idx = np.array([j for j, _ in exp[key]], dtype=np.int64)
            out.append((region, idx, np.array([hexf(b) for _, b in exp[key]], dtype=np.float32)))
    if full is not None and name + ".f32" in full.files:
        ref = full[name + ".f32"]
        out.append(("f32", np.arange(ref.size), ref))
    return out


def load_cases():
    with open(os.path.join(GOLDEN, "krum_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    return np.load(os.path.join(GOLDEN, "krum_full_small.npz"), allow_pickle=False)
