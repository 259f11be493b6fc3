"""Generate the Multi-Krum fixtures from the reference (TL-System/plato, examples/detector).

    python tests/golden/make_golden_krum.py --reference /path/to/plato

Runs ``aggregations.get()`` of examples/detector/aggregations.py with
``Config().server.secure_aggregation_type = "Multi-krum"`` on inputs from the counter generator
(``oracle.synth``, replayed by tests/krum_cases.build_inputs) and writes

    tests/golden/krum_cases.json       recipe, the reference's selection order, SHA-256 of its outputs,
                                       dtypes, samples
    tests/golden/krum_full_small.npz   full outputs of two lenet5 cases

The reference's selection order is read off its own ``torch.argsort`` calls (one per selection step;
the pick is element 0 of the result, an index into the clients still remaining).

Separation: at every selection step the scores are recomputed in float64 and the relative gap between
the smallest and the second smallest must exceed 2 * D * 2^-24, the worst-case fp32 summation bound of
the reference's own distances (lenet5: D = 61,706, 7.4e-3), so that no rounding of either side can
change a pick.  For ResNet-18 (D = 11.2e6) that bound is vacuous (> 1); the generator requires a gap
>= 0.05 there, which is a practical margin and not a proof.  A recipe that fails the condition gets
another seed here, never a looser condition.

ResNet-18 stops at K = 8: the reference's flatten_weights is quadratic in copies.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import boot_reference, canon, layout_of, sha  # noqa: E402,F401

from tests import krum_cases as kc  # noqa: E402
from tests import krum_oracle as ko  # noqa: E402


def recipes():
    # seeds: 300 + K, but K = 64 (seeds 364..367 miss the separation condition at one of the late steps)
    out = [{"name": f"mkrum_lenet5_k{k}", "model": "lenet5", "k": k, "seed": {64: 368}.get(k, 300 + k), "f": kc.F}
           for k in kc.KS_LENET]
    # seeds 408..411 give gaps of 0.014..0.042 (the 20 counters add a few large random terms): 412 is the first >= 0.05
    out.append({"name": "mkrum_resnet18_k8", "model": "resnet18", "k": 8, "seed": 412, "f": kc.F})
    return out


def exact_sqdist(xf, xi):
    """float64 distances of the fp32 inputs with exact (float64) differences."""
    c = ko.columns(xf, xi).astype(np.float64)
    k = c.shape[0]
    out = np.zeros((k, k))
    for i in range(k):
        for j in range(i + 1, k):
            d = c[i] - c[j]
            out[i, j] = out[j, i] = float(np.dot(d, d))
    return out


def min_gap(dist, f, required):
    """The smallest relative gap between the two lowest scores over the selection steps; asserts it."""
    remaining, worst = list(range(dist.shape[0])), np.inf
    while len(remaining) > 2 * f + 2:
        s = ko.scores_of(dist, remaining, f)
        lo = np.argsort(s, kind="stable")
        gap = (s[lo[1]] - s[lo[0]]) / s[lo[0]]
        assert gap > required, f"scores too close at m = {len(remaining)}: gap {gap:.3e} <= {required:.3e}"
        worst = min(worst, gap)
        remaining.pop(int(lo[0]))
    return float(worst)


class _TorchSpy:
    """The torch module with ``argsort`` recorded (aggregations.py calls it once per selection step)."""

    def __init__(self, torch):
        self._torch, self.picks = torch, []

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def argsort(self, *args, **kwargs):
        out = self._torch.argsort(*args, **kwargs)
        self.picks.append(int(out[0]))
        return out


def run_case(recipe, aggregations, full):
    import torch

    layout, xf, xi = kc.build_inputs(recipe)
    d = layout.n_f32 + layout.n_i64
    required = 2 * d * 2.0 ** -24
    if required >= 1:  # vacuous at this size: a practical margin instead (see the module docstring)
        required = 0.05
    recipe["required_gap"] = required
    recipe["min_gap"] = min_gap(exact_sqdist(xf, xi), recipe["f"], required)
    payloads = kc.state_dicts(layout, xf, xi)
    entries, nf, ni = layout_of(payloads[0])
    assert (nf, ni) == (layout.n_f32, layout.n_i64)
    spy = _TorchSpy(torch)
    aggregations.torch = spy
    try:
        result = aggregations.get()(None, None, payloads)
    finally:
        aggregations.torch = torch
    assert list(result) == list(payloads[0])
    remaining, selection = list(range(recipe["k"])), []
    for at in spy.picks:
        selection.append(remaining.pop(at))
    assert len(selection) == recipe["k"] - 2 * recipe["f"] - 2
    assert selection != list(range(len(selection))), "the permutation left the selection in identity order"
    out_f, out_i, dtypes = kc.flat_result(layout, result)
    cf, ci = canon(out_f), canon(out_i)
    sf, si = kc.sample_index(cf.size), kc.sample_index(ci.size)
    if recipe["model"] == "lenet5" and recipe["k"] in kc.FULL_KS:
        full[recipe["name"] + ".f32"] = cf
    return {"recipe": recipe,
            "expected": {"selection": selection, "sha_f32": sha(cf), "sha_i64f": sha(ci), "dtypes": dtypes,
                         "samples_f32": [[int(j), "%08x" % int(cf.view(np.uint32)[j])] for j in sf],
                         "samples_i64f": [[int(j), "%08x" % int(ci.view(np.uint32)[j])] for j in si]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        boot_reference(args.reference, work)
        sys.path.insert(0, os.path.join(args.reference, "examples/detector"))
        from plato.config import Config

        server = dict(Config().server._asdict(), secure_aggregation_type="Multi-krum")
        Config.server = types.SimpleNamespace(**server)
        import aggregations

        full, cases = {}, []
        for recipe in recipes():
            cases.append(run_case(recipe, aggregations, full))
            print(recipe["name"], "gap %.3e (> %.3e)" % (recipe["min_gap"], recipe["required_gap"]),
                  cases[-1]["expected"]["selection"][:8], flush=True)
    with open(os.path.join(HERE, "krum_cases.json"), "w") as f:
        json.dump({"reference": "examples/detector/aggregations.py: multi_krum", "cases": cases}, f, indent=0)
    np.savez(os.path.join(HERE, "krum_full_small.npz"), **full)


if __name__ == "__main__":
    main()
