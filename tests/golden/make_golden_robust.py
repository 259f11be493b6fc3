"""Generate the robust-aggregation fixtures from the reference (TL-System/plato, examples/detector).

    python tests/golden/make_golden_robust.py --reference /path/to/plato

Runs ``aggregations.get()`` of examples/detector/aggregations.py with
``Config().server.secure_aggregation_type = "Median"`` on inputs from the counter generator
(``oracle.synth``, replayed by tests/robust_cases.build_inputs) and writes

    tests/golden/robust_cases.json       recipe, SHA-256 of the canonicalised outputs, dtypes, samples
    tests/golden/robust_full_small.npz   full outputs of a few lenet5 cases

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

from tests import robust_cases as rc  # noqa: E402


def recipes():
    out = [{"name": f"median_lenet5_k{k}", "model": "lenet5", "k": k, "seed": 100 + k} for k in rc.KS_LENET]
    out.append({"name": "median_resnet18_k8", "model": "resnet18", "k": 8, "seed": 208})
    return out


def run_case(recipe, aggregations, full):
    from plato_amd.arena import ArenaLayout

    layout = ArenaLayout.from_shapes(rc.model_spec(recipe["model"]))
    recipe["overrides"], recipe["mixed_zero"] = rc.overrides_for(recipe["k"], layout.n_f32, layout.n_i64)
    layout, xf, xi = rc.build_inputs(recipe)
    payloads = rc.state_dicts(layout, xf, xi)
    entries, nf, ni = layout_of(payloads[0])
    assert (nf, ni) == (layout.n_f32, layout.n_i64)
    result = aggregations.get()(None, None, payloads)
    assert list(result) == list(payloads[0])
    out_f, out_i, dtypes = rc.flat_result(layout, result)
    cf, ci = rc.canon_case(out_f, recipe["mixed_zero"]), canon(out_i)
    sf, si = rc.sample_index(cf.size), rc.sample_index(ci.size)
    if recipe["model"] == "lenet5" and recipe["k"] in rc.FULL_KS:
        full[recipe["name"] + ".f32"] = cf
    return {"recipe": recipe,
            "expected": {"sha_f32": sha(cf), "sha_i64f": sha(ci), "dtypes": dtypes,
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

        server = dict(Config().server._asdict(), secure_aggregation_type="Median")
        Config.server = types.SimpleNamespace(**server)
        import aggregations

        full, cases = {}, []
        for recipe in recipes():
            cases.append(run_case(recipe, aggregations, full))
            print(recipe["name"], cases[-1]["expected"]["sha_f32"][:12], flush=True)
    with open(os.path.join(HERE, "robust_cases.json"), "w") as f:
        json.dump({"reference": "examples/detector/aggregations.py: median", "cases": cases}, f, indent=0)
    np.savez(os.path.join(HERE, "robust_full_small.npz"), **full)


if __name__ == "__main__":
    main()
