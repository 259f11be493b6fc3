"""Generate the FLDetector fixtures from the reference (TL-System/plato, examples/detector).

    python tests/golden/make_golden_fldetector.py --reference /path/to/plato

Drives ``detectors.fl_detector`` of examples/detector/detectors.py through the scenarios of
tests/fldetector_cases.py, round after round, in a temporary working directory (the reference pickles its
record to ``./record<pid>.pkl`` there) with ``np.random.seed`` set before every call (its k-means draws
its initial centres from numpy's global generator).  It is called as the detector server calls it:
``fl_detector(baseline_weights, weights_attacked, deltas_attacked, received_ids, received_staleness)``.
Writes

    tests/golden/fldetector_cases.json       per scenario and round: the ids in arrival order, the reference's
                                             unnormalised distances (a spy on its torch.norm), its normalised
                                             distances and malicious_ids, the float64 evaluation of its own
                                             formula on the same fp32 inputs (``exact``), ``ref_err`` =
                                             max_k |ref_k - exact_k| / exact_k, and the system's condition
    tests/golden/fldetector_full_small.npz   the reference's record: its S and Y rows after the last round
                                             and its last_gradients after every round (state-dict order)

Asserted for every round, and a scenario whose seed fails an assertion is generated again with another:
    - cond(mat) < 1e6: ``exact`` is exact to far below fp32 resolution;
    - tests/fldetector_oracle.py started from the reference's record is within ref_err / 2 of ``exact``;
    - the reference's malicious_ids are ``two_means_1d`` of its own scores;
    - the lowest flagged score exceeds the highest clean score by at least a quarter of the score range.
"""

from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import boot_reference, f32hex  # noqa: E402

from plato_amd import detectors as host  # noqa: E402
from tests import fldetector_cases as fc  # noqa: E402
from tests import fldetector_oracle as fo  # noqa: E402


class _TorchSpy:
    """The torch module with the results of ``norm`` recorded."""

    def __init__(self, torch):
        self._torch, self.norms = torch, []

    def __getattr__(self, name):
        fn = getattr(self._torch, name)
        if name != "norm":
            return fn

        def recorded(*args, **kwargs):
            out = fn(*args, **kwargs)
            self.norms.append(out.detach().clone())
            return out

        return recorded


def exact_distances(s_rows, y_rows, last_w, last_g, weights, deltas):
    """The reference's formula (lbfgs() and the norm of detectors.py:359-364) in float64 on its own fp32
    inputs; returns (distances [K], cond(mat))."""
    d = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    s, y = d(np.stack(s_rows)), d(np.stack(y_rows))
    sy, ss = s @ y.T, s @ s.T
    low = sy - np.triu(sy)
    sigma = (s[-1] @ y[-1]) / (y[-1] @ y[-1])
    mat = np.block([[sigma * ss, low], [low.T, -np.diag(np.diag(sy))]])
    v = np.mean(d((weights - last_w[None, :]).astype(np.float32)), axis=0)
    p = np.concatenate([s @ (sigma * v), y @ v])
    hvp = sigma * v - np.concatenate([sigma * s.T, y.T], axis=1) @ np.linalg.solve(mat, p)
    pred = d(last_g) + hvp
    return np.sqrt(np.sum((pred[None, :] - d(deltas)) ** 2, axis=1)), float(np.linalg.cond(mat))


def run_scenario(recipe, ref, torch):
    lay = fc.layout_of(recipe)
    index = host.arena_index(lay)
    rounds = fc.build_scenario(recipe)
    record_path = "./record" + str(os.getpid()) + ".pkl"
    if os.path.exists(record_path):
        os.remove(record_path)
    oracle_own = fo.Record(index.size)
    out, record, last_g_rows = [], None, []
    for t, (bf, bi, xf, xi, ids) in enumerate(rounds):
        baseline = fc.state_dict(lay, bf, bi)
        payloads = [fc.state_dict(lay, xf[c], xi[c]) for c in range(recipe["k"])]
        deltas = [type(p)((n, p[n] - baseline[n]) for n in p) for p in payloads]  # compute_weight_deltas
        flat_w = ref.flatten_weights(payloads).numpy()
        flat_d = ref.flatten_weights(deltas).numpy()
        spy = _TorchSpy(torch)
        ref.torch = spy
        np.random.seed(recipe["seed"] + t)
        try:
            malicious, approved = ref.fl_detector(baseline, payloads, deltas, ids, [0] * len(ids))
        finally:
            ref.torch = torch
        entry = {"ids": ids, "malicious": [int(i) for i in malicious], "distances": None, "normalised": None}
        own = oracle_own.round(xf, xi, bf, bi, ids)
        if t:
            s_rows, y_rows, last_w, last_g, scores = record
            assert len(spy.norms) == 1
            ref_dist = spy.norms[0].numpy().astype(np.float32)
            exact, cond = exact_distances([r.numpy() for r in s_rows], [r.numpy() for r in y_rows], last_w.numpy(),
                                          last_g.numpy(), flat_w, flat_d)
            ref_err = float(np.max(np.abs(ref_dist.astype(np.float64) - exact) / exact))
            if not cond < 1e6:
                return None, f"round {t}: cond {cond:.3g}"
            rec = fo.Record.from_reference([r.numpy() for r in s_rows], [r.numpy() for r in y_rows], last_w.numpy(),
                                           last_g.numpy(), scores, index)
            mine = rec.round(xf, xi, bf, bi, ids)
            err = float(np.max(np.abs(np.sqrt(mine["d2"]) - exact) / exact))
            if not err <= ref_err / 2:
                return None, f"round {t}: oracle err {err:.3g} against ref_err {ref_err:.3g}"
            normalised = ref_dist / np.sum(ref_dist)
            ref_scores = np.array([host.history_score([v for v in scores[c] if v is not None], dn)
                                   for c, dn in zip(ids, normalised)], dtype=np.float32)
            flagged, clean = host.two_means_1d(ref_scores)
            if flagged != sorted(entry["malicious"]):
                return None, f"round {t}: k-means {sorted(entry['malicious'])}, exact split {flagged}"
            span = float(ref_scores.max() - ref_scores.min())
            gap = float(ref_scores[flagged].min() - ref_scores[clean].max())
            if not gap >= span / 4:
                return None, f"round {t}: gap {gap:.3g} of range {span:.3g}"
            if own["malicious"] != flagged:
                return None, f"round {t}: the oracle's own record flags {own['malicious']}, the reference {flagged}"
            entry.update(distances=[f32hex(v) for v in ref_dist], normalised=[f32hex(v) for v in normalised],
                         exact=[float(v).hex() for v in exact], ref_err=ref_err, oracle_err=err, cond=cond,
                         gap_over_range=gap / span,
                         own_score_diff=float(np.max(np.abs(own["scores"].astype(np.float64) - ref_scores))))
        else:
            assert entry["malicious"] == [] and len(approved) == len(payloads) and not spy.norms
        with open(record_path, "rb") as f:
            record = [pickle.load(f) for _ in range(5)]
        # what the reference stored for this round's clients is what the fixture replays
        for c, dn in zip(ids, entry["normalised"] or [None] * len(ids)):
            stored = record[4][c][-1]
            assert (stored is None) if dn is None else (f32hex(stored) == dn)
        last_g_rows.append(record[3].numpy().copy())
        out.append(entry)
    name = recipe["name"]
    full = {name + ".S": np.stack([r.numpy() for r in record[0]]), name + ".Y": np.stack([r.numpy() for r in record[1]]),
            name + ".G": np.stack(last_g_rows)}
    return ({"recipe": recipe, "rounds": out}, full), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    full, cases = {}, []
    with tempfile.TemporaryDirectory() as work:
        boot_reference(args.reference, work)
        os.chdir(work)  # the reference writes app.log on import and its record on every call
        sys.path.insert(0, os.path.join(args.reference, "examples/detector"))
        import torch

        import detectors as ref

        for recipe in fc.recipes():
            for attempt in range(8):
                tried = dict(recipe, seed=recipe["seed"] + attempt)
                got, why = run_scenario(tried, ref, torch)
                if got is not None:
                    break
                print(recipe["name"], "seed", tried["seed"], "replaced:", why, flush=True)
            else:
                raise AssertionError(f"{recipe['name']}: no seed passes the generator's assertions")
            if tried["seed"] != recipe["seed"]:
                raise AssertionError(f"{recipe['name']}: put seed {tried['seed']} into tests/fldetector_cases.recipes()")
            cases.append(got[0])
            full.update(got[1])
            rs = got[0]["rounds"][1:]
            print(recipe["name"], "cond %.3g..%.3g" % (min(r["cond"] for r in rs), max(r["cond"] for r in rs)),
                  "ref_err %.3g..%.3g" % (min(r["ref_err"] for r in rs), max(r["ref_err"] for r in rs)),
                  "oracle_err max %.3g" % max(r["oracle_err"] for r in rs),
                  "own score diff max %.3g" % max(r["own_score_diff"] for r in rs),
                  "flagged", [r["malicious"] for r in rs], flush=True)
        os.chdir(ROOT)
    with open(os.path.join(HERE, "fldetector_cases.json"), "w") as f:
        json.dump({"reference": "examples/detector/detectors.py: fl_detector, lbfgs", "cases": cases}, f, indent=0)
    np.savez(os.path.join(HERE, "fldetector_full_small.npz"), **full)


if __name__ == "__main__":
    main()
