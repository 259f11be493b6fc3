"""Loading and replaying the reference-generated robust-aggregation cases (tests/golden/robust_*).

A case = recipe (model, K, seed, overrides, the mixed-zero column indices) + what the reference's
``aggregations.median`` produced: SHA-256 of the canonicalised fp32 and int64-as-fp32 outputs, the
result dtypes, 64 sampled values, and full arrays for a few lenet5 cases.  The inputs are rebuilt from
``oracle.synth`` by :func:`build_inputs`, shared with the generator (tests/golden/make_golden_robust.py).

Mixed-zero columns hold both -0 and +0 with a zero median: the reference returns whichever sign its
selection met (the two compare equal), the kernel's total order puts -0 first.  They are listed by
index, compared by value, and written as +0 before a digest is taken (:func:`canon_case`).
"""

from __future__ import annotations

import json
import os

import numpy as np

from tests.golden_cases import GOLDEN, canon, model_spec, sha  # noqa: F401

KS_LENET = (1, 2, 3, 5, 8, 16, 33, 128, 256)
FULL_KS = (3, 16, 256)  # lenet5 cases with full arrays (a committed file stays under 1 MiB)
N_SAMPLES = 64
NEG_ZERO, POS_ZERO = 0x80000000, 0x00000000


def overrides_for(k: int, n_f32: int, n_i64: int):
    """([client, region, index, value] bit overrides, the mixed-zero fp32 indices) of a case."""
    assert n_f32 >= 8
    ov = [[0, "f32", 0, "7fc00000"],          # one NaN in the column
          [0, "f32", 1, "7f800000"],          # a +inf
          [0, "f32", 2, "ff800000"]]          # a -inf
    for c in range(k):
        ov.append([c, "f32", 3, "%08x" % (((c & 1) << 31) | (c + 1))])          # subnormals of both signs
        ov.append([c, "f32", 4, "3fc00000"])                                   # all equal
        ov.append([c, "f32", 5, "3f400000" if c % 4 == 3 else "3f000000"])     # duplicates across the median
        ov.append([c, "f32", 6, "%08x" % (NEG_ZERO if c % 2 == 0 else POS_ZERO)])
        ov.append([c, "f32", 7, "%08x" % (NEG_ZERO if c == 0 else POS_ZERO)])
        if n_i64:
            ov.append([c, "i64", 0, str((1 << 24) + 1 + 2 * c)])              # above 2^24: the cast rounds
    return ov, [6, 7]


def build_inputs(recipe):
    """(layout, X_f32 [K, n_f32] float32, X_i64 [K, n_i64] int64) of a recipe, overrides applied."""
    from oracle import synth
    from plato_amd.arena import ArenaLayout

    layout = ArenaLayout.from_shapes(model_spec(recipe["model"]))
    k, seed = recipe["k"], recipe["seed"]
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, seed)
    xs = [synth.client_arena(bf, bi, seed, c) for c in range(k)]
    xf = np.stack([x[0] for x in xs]).astype(np.float32)
    xi = np.stack([x[1] for x in xs]).astype(np.int64)
    for c, region, idx, val in recipe["overrides"]:
        if region == "f32":
            xf.view(np.uint32)[c, idx] = np.uint32(int(val, 16))
        else:
            xi[c, idx] = np.int64(int(val))
    return layout, xf, xi


def state_dicts(layout, xf, xi):
    import torch

    return [layout.unpack(torch.from_numpy(xf[c]), torch.from_numpy(xi[c])) for c in range(xf.shape[0])]


def canon_case(a: np.ndarray, mixed_zero) -> np.ndarray:
    """NaN-canonicalised copy with the mixed-zero columns' zeros written as +0."""
    a = canon(a)
    for j in mixed_zero:
        if a[j] == 0:
            a.view(np.uint32)[j] = POS_ZERO
    return a


def mixed_zero_columns(xf: np.ndarray, med: np.ndarray) -> np.ndarray:
    """Indices of the columns that hold both zero signs and have a zero median."""
    u = xf.view(np.uint32)
    both = (u == np.uint32(NEG_ZERO)).any(axis=0) & (u == np.uint32(POS_ZERO)).any(axis=0)
    return np.flatnonzero(both & (med == 0))


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


def load_cases():
    with open(os.path.join(GOLDEN, "robust_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    return np.load(os.path.join(GOLDEN, "robust_full_small.npz"), allow_pickle=False)
