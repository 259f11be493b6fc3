"""The seeded FLDetector scenarios and their reference-generated fixtures (tests/golden/fldetector_*).

A scenario is a small federated run of several rounds: a quadratic objective with a diagonal Hessian, K
clients with optima of their own, a fixed sequence of global models w_t (the mean benign step), and from
round 1 on A clients that send the negated, tripled step.  Every number comes from ``oracle.synth``'s
counter generator and float64 numpy arithmetic rounded to fp32 once, so the generator
(tests/golden/make_golden_fldetector.py), the CPU tests and the GPU tests rebuild the same bits.  Models
with int64 entries carry counters that every client advances by the same amount, one client by one more.

The fixture keeps, per round, what the reference's ``detectors.fl_detector`` produced (its unnormalised
distances and ``malicious_ids``), the float64 evaluation of its formula on the same fp32 inputs
(``exact``) and the reference's own error against it (``ref_err``); the npz keeps the reference's record
(its S and Y rows and ``last_gradients`` per round, in state-dict order).
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np

from tests.golden_cases import GOLDEN, hexf  # noqa: F401

MLP = [("fc1.weight", (24, 40), "f32"), ("fc1.bias", (24,), "f32"), ("fc2.weight", (10, 24), "f32"),
       ("fc2.bias", (10,), "f32")]
# two BatchNorm layers and a step counter: int64 entries between the fp32 ones (the arena order differs
# from the state-dict order)
BN = [("conv1.weight", (8, 3, 3, 3), "f32"), ("bn1.weight", (8,), "f32"), ("bn1.bias", (8,), "f32"),
      ("bn1.running_mean", (8,), "f32"), ("bn1.running_var", (8,), "f32"), ("bn1.num_batches_tracked", (), "i64"),
      ("conv2.weight", (5, 8, 3, 3), "f32"), ("bn2.weight", (5,), "f32"), ("bn2.bias", (5,), "f32"),
      ("bn2.running_mean", (5,), "f32"), ("bn2.running_var", (5,), "f32"), ("bn2.num_batches_tracked", (), "i64"),
      ("steps", (3,), "i64"), ("fc.weight", (10, 5), "f32"), ("fc.bias", (10,), "f32")]
# several reduction chunks with a ragged last one in the fp32 region
WIDE = [("conv.weight", (16, 8, 3, 3), "f32"), ("bn.weight", (16,), "f32"), ("bn.bias", (16,), "f32"),
        ("bn.running_mean", (16,), "f32"), ("bn.running_var", (16,), "f32"), ("bn.num_batches_tracked", (), "i64"),
        ("fc.weight", (10, 340), "f32"), ("fc.bias", (10,), "f32")]
SPECS = {"mlp": MLP, "bn": BN, "wide": WIDE}

LR = 0.3


def recipes():
    def one(model, k, attackers, rounds, seed):
        return {"name": f"fld_{model}_k{k}_a{len(attackers)}", "model": model, "k": k, "attackers": list(attackers),
                "rounds": rounds, "seed": seed}

    # attackers are client ids (1-based, as the reference's); with none, client 1 is a benign outlier
    return [one("bn", 8, (2, 7), 8, 9100), one("mlp", 3, (2,), 6, 9200), one("mlp", 9, (), 6, 9300),
            one("bn", 9, (4,), 6, 9400), one("wide", 8, (1, 6), 7, 9500)]


def layout_of(recipe):
    from plato_amd.arena import ArenaLayout

    return ArenaLayout.from_shapes(SPECS[recipe["model"]])


def _u(n, seed, stream):
    """n float64 values uniform on (-1, 1) (a 2^-23 grid) from the counter generator."""
    from oracle import synth

    return synth.synth_f32(n, seed, stream, -23).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _scenario(name):
    recipe = next(r for r in recipes() if r["name"] == name)
    return build_scenario(recipe)


def build_scenario(recipe):
    """[(baseline fp32 [n_f32], baseline int64 [n_i64], X_f32 [K, n_f32], X_i64 [K, n_i64], ids [K])] per round:
    the payloads of a round in arrival order, ``ids`` their client ids.  Arrays are read-only."""
    lay = layout_of(recipe)
    nf, ni, k, seed = lay.n_f32, lay.n_i64, recipe["k"], recipe["seed"]
    hess = 0.5 + 0.5 * np.abs(_u(nf, seed, 1))
    opt = _u(nf, seed, 2)
    spread = [0.3 * (6.0 if (not recipe["attackers"] and c == 0) else 1.0) for c in range(k)]
    local = [opt + spread[c] * _u(nf, seed, 10 + c) for c in range(k)]
    w = (0.0625 * _u(nf, seed, 3)).astype(np.float32)
    wi = np.arange(2, 2 + ni, dtype=np.int64)
    rounds = []
    for t in range(recipe["rounds"]):
        xf = np.empty((k, nf), dtype=np.float32)
        xi = np.empty((k, ni), dtype=np.int64)
        steps = []
        for c in range(k):
            step = -LR * hess * (w.astype(np.float64) - local[c]) + 0.02 * _u(nf, seed, 1000 * (t + 1) + c)
            bad = (c + 1) in recipe["attackers"] and t >= 1
            if not bad:
                steps.append(step)
            xf[c] = (w.astype(np.float64) + (-3.0 * step if bad else step)).astype(np.float32)
            xi[c] = wi + 1 + (1 if c == (t % k) else 0)
        order = np.roll(np.arange(k), t)  # arrival order changes from round to round
        ids = [int(c) + 1 for c in order]
        out = (w.copy(), wi.copy(), xf[order], xi[order], ids)
        for a in out[:4]:
            a.setflags(write=False)
        rounds.append(out)
        w = (w.astype(np.float64) + np.mean(steps, axis=0)).astype(np.float32)
        wi = wi + 1
    return rounds


def scenario(name):
    return _scenario(name)


def state_dict(layout, f32: np.ndarray, i64: np.ndarray):
    import torch

    return layout.unpack(torch.from_numpy(f32.copy()), torch.from_numpy(i64.copy()))


def hexes(values) -> np.ndarray:
    return np.array([hexf(b) for b in values], dtype=np.float32)


def f64s(values) -> np.ndarray:
    return np.array([float.fromhex(v) for v in values], dtype=np.float64)


def load_cases():
    with open(os.path.join(GOLDEN, "fldetector_cases.json")) as f:
        return json.load(f)["cases"]


def load_full():
    return np.load(os.path.join(GOLDEN, "fldetector_full_small.npz"), allow_pickle=False)


def reference_record(case, full, t, layout):
    """The reference's five record objects as it pickled them after round t - 1 (what its round t loads):
    (S rows, Y rows, last_weights, last_gradients, malicious_score_dict), flat vectors in state-dict
    order as float32 arrays."""
    name = case["recipe"]["name"]
    s, y, g = full[name + ".S"], full[name + ".Y"], full[name + ".G"]
    bf, bi = scenario(name)[t - 1][:2]
    # flatten_weight of the baseline: state-dict order, the counters promoted by torch.cat
    last_w = np.concatenate([v.reshape(-1).numpy().astype(np.float32) for v in state_dict(layout, bf, bi).values()])
    scores: dict = {}
    for r in case["rounds"][:t]:
        dist = [None] * len(r["ids"]) if r["normalised"] is None else list(hexes(r["normalised"]))
        for cid, d in zip(r["ids"], dist):
            scores.setdefault(cid, []).append(d)
    return list(s[:t]), list(y[:t]), last_w, g[t - 1], scores
