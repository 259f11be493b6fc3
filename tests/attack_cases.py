"""Loading and replaying the reference-generated attack cases (tests/golden/attack_*).

A case = recipe (model, attack, A, seed, the attack's parameter) + what the reference's ``attacks.get()``
produced on it: SHA-256 of every attacker's poisoned payload, the poison vector and the vector it came from
(std, mean or average) as digests and sampled values, full vectors for a few small cases, and for the
searches the reference's lambda, norm and threshold with the interval a float64 search lands in.  The inputs
are rebuilt from ``oracle.synth`` by :func:`build_inputs`, shared with the generator
(tests/golden/make_golden_attacks.py).
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np

from tests.golden_cases import GOLDEN, canon, hexf, model_spec, sha  # noqa: F401

AS_LENET = (2, 3, 5, 20)
PER_ROUNDS = (10, 100)
LAMBADA = 2  # the value every config of the example ships
N_SAMPLES = 64
ATTACK_TYPE = {"lie": "LIE", "lambda": "Lambda_attack", "minmax": "Min-Max", "minsum": "Min-Sum"}
#: cases whose vector (std, mean, average) is stored whole (a committed file stays under 1 MiB)
FULL = ("lambda_lenet5_a5", "minmax_lenet5_a5", "minsum_lenet5_a5")

# a model with int64 counters small enough to store whole: two BatchNorm layers and a step counter
BN_TOY = [("conv1.weight", (8, 3, 3, 3), "f32"), ("bn1.weight", (8,), "f32"), ("bn1.bias", (8,), "f32"),
          ("bn1.running_mean", (8,), "f32"), ("bn1.running_var", (8,), "f32"), ("bn1.num_batches_tracked", (), "i64"),
          ("conv2.weight", (5, 8, 3, 3), "f32"), ("bn2.weight", (5,), "f32"), ("bn2.bias", (5,), "f32"),
          ("bn2.running_mean", (5,), "f32"), ("bn2.running_var", (5,), "f32"), ("bn2.num_batches_tracked", (), "i64"),
          ("steps", (3,), "i64"), ("fc.weight", (10, 5), "f32"), ("fc.bias", (10,), "f32")]


def recipes():
    out = []

    def add(kind, model, a, seed, **params):
        name = f"{kind}_{model}_a{a}" + (f"_n{params['per_round']}" if kind == "lie" else "")
        out.append(dict(name=name, kind=kind, model=model, a=a, seed=seed, **params))

    for at, a in enumerate(AS_LENET):
        for per_round in PER_ROUNDS:
            add("lie", "lenet5", a, 4100 + at, per_round=per_round)
        add("lambda", "lenet5", a, 4200 + at, lambada_value=LAMBADA)
        add("minmax", "lenet5", a, 4300 + at)
        add("minsum", "lenet5", a, 4400 + at)
    add("lie", "bn_toy", 3, 4500, per_round=100)
    add("lie", "bn_toy", 1, 4501, per_round=100)  # the solo attacker: nothing changes
    add("lambda", "bn_toy", 3, 4502, lambada_value=LAMBADA)
    add("minmax", "bn_toy", 3, 4503)
    add("minsum", "bn_toy", 3, 4504)
    return out


def spec_of(model: str):
    return BN_TOY if model == "bn_toy" else model_spec(model)


def build_inputs(recipe):
    """(layout, baseline fp32, baseline int64, W_f32 [A, n_f32], W_i64 [A, n_i64]) of a recipe."""
    from oracle import synth
    from plato_amd.arena import ArenaLayout

    layout = ArenaLayout.from_shapes(spec_of(recipe["model"]))
    a, seed = recipe["a"], recipe["seed"]
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, seed)
    wf = np.empty((a, layout.n_f32), dtype=np.float32)
    wi = np.empty((a, layout.n_i64), dtype=np.int64)
    for c in range(a):
        wf[c], wi[c] = synth.client_arena(bf, bi, seed, c)
    return layout, bf, bi, wf, wi


def state_dict(layout, f32: np.ndarray, i64: np.ndarray):
    import torch

    return layout.unpack(torch.from_numpy(f32.copy()), torch.from_numpy(i64.copy()))


def flat_payload(layout, payload):
    """(fp32 region float32, int64 region int64) of a payload in arena order."""
    f = [payload[e.name].reshape(-1).numpy() for e in layout.entries if e.region == "f32"]
    i = [payload[e.name].reshape(-1).numpy() for e in layout.entries if e.region == "i64"]
    return (np.concatenate(f) if f else np.zeros(0, dtype=np.float32),
            np.concatenate(i) if i else np.zeros(0, dtype=np.int64))


def sample_index(n: int) -> np.ndarray:
    return np.unique(np.concatenate([np.arange(min(n, 8)), np.linspace(0, n - 1, N_SAMPLES - 8).astype(np.int64)])
                     ) if n else np.zeros(0, dtype=np.int64)


def samples(v: np.ndarray):
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return [[int(j), "%08x" % int(bits[j])] for j in sample_index(v.size)]


def sampled(entry):
    """(indices, float32 values) of a stored sample list."""
    idx = np.array([j for j, _ in entry], dtype=np.int64)
    return idx, np.array([hexf(b) for _, b in entry], dtype=np.float32)


def row_digest(f32: np.ndarray, i64: np.ndarray) -> str:
    return sha(canon(f32)) + ":" + sha(np.ascontiguousarray(i64, dtype=np.int64))


def load_cases():
    with open(os.path.join(GOLDEN, "attack_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    return np.load(os.path.join(GOLDEN, "attack_full_small.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def cases():
    return load_cases()


def names():
    return [c["recipe"]["name"] for c in cases()]


def case_of(name):
    return cases()[names().index(name)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(layout, bf, bi, wf, wi, delta columns) of a case; shared among the tests and read-only."""
    from tests import attack_oracle as ao

    layout, bf, bi, wf, wi = build_inputs(case_of(name)["recipe"])
    u = ao.columns((wf - bf[None, :]).astype(np.float32), wi - bi[None, :])
    for arr in (bf, bi, wf, wi, u):
        arr.setflags(write=False)
    return layout, bf, bi, wf, wi, u
