"""Generate the Bulyan and Trimmed-mean fixtures from the reference (TL-System/plato, examples/detector).

    python tests/golden/make_golden_bulyan.py --reference /path/to/plato

Runs ``aggregations.get()`` of examples/detector/aggregations.py with
``Config().server.secure_aggregation_type`` = "Bulyan" or "Trimmed-mean", ``clients.total_clients = K``
and ``clients.attacker_ids`` of length f, on inputs from the counter generator (``oracle.synth``,
replayed by tests/krum_cases.build_inputs) and writes

    tests/golden/bulyan_cases.json       recipe, the reference's selection order, SHA-256 of its outputs,
                                         dtypes, samples, the boundary-tie columns
    tests/golden/bulyan_full_small.npz   full outputs of three lenet5 cases

The reference's selection order is read off its own 1-D ``torch.argsort`` calls (one per selection
step; the pick is element 0, an index into the clients still remaining).  ``bulyan`` and
``trimmed_mean`` also call ``argsort`` on the 2-D |x - median|: those calls are not counted.

Separation: at every selection step that sums three or more distances, the condition of
make_golden_krum.py (relative gap of the two lowest float64 scores > 2 * D * 2^-24; >= 0.05 where that
is vacuous).  Two kinds of step tie exactly by construction, in the reference as in the product, and no
seed can separate them:
  * a step that sums one term sums the diagonal's exact +0 for every client: all scores tie;
  * a step that sums two terms scores a client by 0 + the distance to its nearest neighbour, so the two
    clients of the closest pair always share the lowest score, bit for bit (fp32 a - b and b - a differ
    in sign only; the device matrix is bitwise symmetric).  The separation condition is asserted there
    between that pair and the third lowest score.
At both the product picks the lowest remaining index among the tied, and the generator asserts that the
reference did too (its argsort of at most 7 scores keeps equal ones in order).  Such steps have
m = f + 3 and m = f + 4 remaining clients and occur for f <= 3 only.

Boundary ties: a column where the b-th and (b+1)-th smallest |x - median| are equal but belong to
different values may keep another value in the reference than under the table-order rule.  They are
listed in the recipe; a lenet5 case may have at most 8, and no stored ResNet-18 sample may be one.  A
recipe that misses a condition gets another seed here, never a looser condition.

The ResNet-18 Bulyan recipe is (K, f) = (6, 1), not (13, 3): see tests/bulyan_cases.py (no seed meets the
0.05 gap there; ``--search`` below reproduces that).
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
from make_golden_krum import exact_sqdist  # noqa: E402

from tests import bulyan_cases as bc  # noqa: E402
from tests import krum_oracle as ko  # noqa: E402
from tests import nearest_oracle as no  # noqa: E402

# name -> seed, where 500 + K (Bulyan) or 600 + K (Trimmed-mean) misses a condition
SEEDS = {"bulyan_lenet5_k64_f5": 565,   # 564: gap 6.8e-3 <= 7.4e-3 at m = 11
         "bulyan_resnet18_k6_f1": 507}  # 506: gap 1.4e-2 <= 0.05 at m = 6


def recipes():
    out = []
    for model, pairs in (("lenet5", bc.BULYAN_LENET), ("resnet18", bc.BULYAN_RESNET)):
        for k, f in pairs:
            name = f"bulyan_{model}_k{k}_f{f}"
            out.append({"name": name, "kind": "Bulyan", "model": model, "k": k, "seed": SEEDS.get(name, 500 + k), "f": f})
    for model, ks in (("lenet5", bc.TRIMMED_LENET), ("resnet18", bc.TRIMMED_RESNET)):
        for k in ks:
            name = f"trimmed_{model}_k{k}"
            out.append({"name": name, "kind": "Trimmed-mean", "model": model, "k": k, "seed": SEEDS.get(name, 600 + k),
                        "f": 0})
    return out


def min_gap(dist, f, required):
    """The smallest relative gap asserted over the selection steps, and {step: remaining index} of the
    steps whose lowest scores tie exactly by construction (see the module docstring)."""
    k = dist.shape[0]
    remaining, worst, tied = list(range(k)), np.inf, {}
    for step in range(no.bulyan_theta(k, f)):
        m = len(remaining)
        s = ko.scores_of(dist, remaining, f)
        lo = np.argsort(s, kind="stable")
        if m - 2 - f == 1:
            assert not s.any() and lo[0] == 0  # the diagonal's +0
            tied[step] = 0
        else:
            first = 0
            if m - 2 - f == 2:  # 0 + the nearest neighbour: the closest pair shares the lowest score
                assert s[lo[0]] == s[lo[1]] and dist[remaining[lo[0]], remaining[lo[1]]] == s[lo[0]]
                tied[step] = int(lo[0])
                first = 1
            gap = (s[lo[first + 1]] - s[lo[first]]) / s[lo[first]]
            assert gap > required, f"scores too close at m = {m}: gap {gap:.3e} <= {required:.3e}"
            worst = min(worst, gap)
        remaining.pop(int(lo[0]))
    return float(worst), tied


def modelled_sqdist(model: str, k: int, seed: int):
    """build_inputs' distance matrix without building the fp32 rows: slot i holds generator client c_i,
    whose noise is uniform in +-2^-7 scaled by s_i = 1 + c_i/8, so the fp32 part of entry [i, j] is
    n_f32 * 2^-14 / 3 * (s_i^2 + s_j^2) up to ~n_f32^-1/2 relative; the counters' part is exact."""
    from oracle import synth
    from plato_amd.arena import ArenaLayout
    from tests.golden_cases import model_spec

    layout = ArenaLayout.from_shapes(model_spec(model))
    perm = bc.kc.permutation(k, seed)
    _, bi = synth.baseline_arena(0, layout.n_i64, seed)
    xi = np.stack([synth.synth_i64(layout.n_i64, seed, int(c) + 1, synth.I64_CLIENT_MOD, add=bi)
                   for c in perm]).astype(np.float64)
    s2 = (1.0 + perm / 8.0) ** 2
    dist = layout.n_f32 * 2.0 ** -14 / 3 * (s2[:, None] + s2[None, :]) + ((xi[:, None] - xi[None]) ** 2).sum(-1)
    dist[np.arange(k), np.arange(k)] = 0.0
    return dist


def search(model: str, k: int, f: int, first: int, last: int, keep: int = 5):
    """Seeds first..last-1 ranked by the smallest gap of min_gap's steps on the modelled matrix; the
    ``keep`` best are then measured on the exact one.  How the seeds in SEEDS and the statement in
    tests/bulyan_cases.py about ResNet-18 at (13, 3) were found:

        --search resnet18:13:3:513:20513    best modelled 0.0494 (seed 10010; exact 0.0494, m = 8)
        --search resnet18:6:1:506:2506
    """
    def worst(dist):
        try:
            return min_gap(dist, f, -np.inf)[0]
        except AssertionError:  # the closest pair is not the tied pair of a two-term step: not usable
            return -np.inf

    ranked = sorted(((worst(modelled_sqdist(model, k, seed)), seed) for seed in range(first, last)), reverse=True)
    for gap, seed in ranked[:keep]:
        _, xf, xi = bc.build_inputs({"model": model, "k": k, "seed": seed})
        print(f"{model} K={k} f={f} seed {seed}: modelled gap {gap:.4f}, exact {worst(exact_sqdist(xf, xi)):.4f}",
              flush=True)


class _TorchSpy:
    """The torch module with the 1-D ``argsort`` calls recorded (one per selection step)."""

    def __init__(self, torch):
        self._torch, self.picks = torch, []

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def argsort(self, *args, **kwargs):
        out = self._torch.argsort(*args, **kwargs)
        if args[0].dim() == 1:
            self.picks.append(int(out[0]))
        return out


def run_case(recipe, aggregations, full, Config):
    import torch

    layout, xf, xi = bc.build_inputs(recipe)
    k, f = recipe["k"], recipe["f"]
    Config.server = types.SimpleNamespace(**dict(vars(Config.server), secure_aggregation_type=recipe["kind"]))
    Config.clients = types.SimpleNamespace(**dict(vars(Config.clients), total_clients=k,
                                                  attacker_ids=list(range(1, f + 1))))
    tied = {}
    if recipe["kind"] == "Bulyan":
        d = layout.n_f32 + layout.n_i64
        required = 2 * d * 2.0 ** -24
        if required >= 1:  # vacuous at this size: a practical margin instead (make_golden_krum.py)
            required = 0.05
        recipe["required_gap"] = required
        recipe["min_gap"], tied = min_gap(exact_sqdist(xf, xi), f, required)
    payloads = bc.state_dicts(layout, xf, xi)
    entries, nf, ni = layout_of(payloads[0])
    assert (nf, ni) == (layout.n_f32, layout.n_i64)
    spy = _TorchSpy(torch)
    aggregations.torch = spy
    try:
        result = aggregations.get()(None, None, payloads)
    finally:
        aggregations.torch = torch
    assert list(result) == list(payloads[0])
    remaining, selection = list(range(k)), []
    if recipe["kind"] == "Bulyan":
        assert len(spy.picks) == no.bulyan_theta(k, f)
        for step, at in enumerate(spy.picks):
            if step in tied:
                assert at == tied[step], f"the reference picked remaining index {at} at a tied step: drop f = {f}"
            selection.append(remaining.pop(at))
        assert selection != list(range(len(selection))), "the permutation left the selection in identity order"
    else:
        assert not spy.picks
    out_f, out_i, dtypes = bc.flat_result(layout, result)
    cf, ci = canon(out_f), canon(out_i)
    sf, si = bc.sample_index(cf.size), bc.sample_index(ci.size)
    tf, ti = bc.tie_columns(recipe, xf, xi, selection)
    recipe["tie_f32"], recipe["tie_i64"] = [int(j) for j in tf], [int(j) for j in ti]
    if recipe["model"] == "lenet5":
        assert tf.size + ti.size <= bc.MAX_TIES_LENET, f"{tf.size + ti.size} boundary-tie columns: another seed"
    else:
        assert not np.intersect1d(tf, sf).size and not np.intersect1d(ti, si).size, "a sample is a tie column"
    if recipe["name"] in bc.FULL:
        full[recipe["name"] + ".f32"] = cf
    return {"recipe": recipe,
            "expected": {"selection": selection, "sha_f32": sha(cf), "sha_i64f": sha(ci), "dtypes": dtypes,
                         "samples_f32": [[int(j), "%08x" % int(cf.view(np.uint32)[j])] for j in sf],
                         "samples_i64f": [[int(j), "%08x" % int(ci.view(np.uint32)[j])] for j in si]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference")
    ap.add_argument("--search", metavar="MODEL:K:F:FIRST:LAST", help="rank seeds by their smallest score gap and exit")
    args = ap.parse_args()
    if args.search:
        model, *numbers = args.search.split(":")
        return search(model, *(int(v) for v in numbers))
    if not args.reference:
        ap.error("--reference is required")
    with tempfile.TemporaryDirectory() as work:
        boot_reference(args.reference, work)
        sys.path.insert(0, os.path.join(args.reference, "examples/detector"))
        from plato.config import Config

        Config.server = types.SimpleNamespace(**Config().server._asdict())
        Config.clients = types.SimpleNamespace(**Config().clients._asdict())
        import aggregations

        full, cases = {}, []
        for recipe in recipes():
            cases.append(run_case(recipe, aggregations, full, Config))
            print(recipe["name"], "gap %.3e" % recipe.get("min_gap", float("nan")), "ties", len(recipe["tie_f32"]),
                  len(recipe["tie_i64"]), cases[-1]["expected"]["selection"][:8], flush=True)
    with open(os.path.join(HERE, "bulyan_cases.json"), "w") as f:
        json.dump({"reference": "examples/detector/aggregations.py: bulyan, trimmed_mean", "cases": cases}, f, indent=0)
    np.savez(os.path.join(HERE, "bulyan_full_small.npz"), **full)


if __name__ == "__main__":
    main()
