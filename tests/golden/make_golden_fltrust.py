"""Generate the Fl-trust fixtures from the reference (TL-System/plato, examples/detector).

    python tests/golden/make_golden_fltrust.py --reference /path/to/plato

Runs ``aggregations.get()`` of examples/detector/aggregations.py with
``Config().server.secure_aggregation_type = "Fl-trust"`` on the inputs of
tests/fltrust_cases.build_inputs and writes

    tests/golden/fltrust_cases.json       recipe, the reference's fp32 scalars as hex, SHA-256 of its
                                          outputs, dtypes, samples, ref_self_err, mean_order_shift
    tests/golden/fltrust_full_small.npz   full outputs of two lenet5 cases

The scalars are read off the reference's own ``torch.dot``, ``torch.norm``, ``torch.mean``,
``torch.maximum`` and ``torch.sum`` calls (a spy in place of its ``torch`` module records every result).
Per client the calls are, in order: K x (dot, norm(mean), norm(x_k)), one maximum, one sum, K x
(norm(x_k + 1e-9), norm(mean)), one sum over the candidates.

Two float64 figures per client, neither from this project's kernels:
    ref_self_err[k]      |reference cos_k - the same formula in float64 on the reference's own mean|:
                         the error of the reference's fp32 dot and norms
    mean_order_shift[k]  |float64 cos_k on the sequential mean - float64 cos_k on the reference's mean|:
                         what the order of the mean's row sum moves

Every recipe that negates clients must have at least that many cosines clipped by the ReLU.

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

from make_golden import boot_reference, canon, f32hex, layout_of, sha  # noqa: E402,F401

from tests import fltrust_cases as fc  # noqa: E402
from tests import fltrust_oracle as fo  # noqa: E402


class _TorchSpy:
    """The torch module with the results of dot, norm, mean, maximum and sum recorded."""

    def __init__(self, torch):
        self._torch, self.calls = torch, []

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _record(self, name, args, kwargs):
        out = getattr(self._torch, name)(*args, **kwargs)
        self.calls.append((name, args[0].detach().clone() if name == "maximum" else None, out.detach().clone()))
        return out

    def dot(self, *a, **k):
        return self._record("dot", a, k)

    def norm(self, *a, **k):
        return self._record("norm", a, k)

    def mean(self, *a, **k):
        return self._record("mean", a, k)

    def maximum(self, *a, **k):
        return self._record("maximum", a, k)

    def sum(self, *a, **k):
        return self._record("sum", a, k)


def region_index(entries, n_f32):
    """For the reference's flat vector (state-dict order): the position of every element in the
    [fp32 region | int64 region] order of this project."""
    parts = []
    for _, region, off, numel, _ in entries:
        parts.append(np.arange(numel) + (off if region == "f32" else n_f32 + off))
    return np.concatenate(parts)


def run_case(recipe, aggregations, full):
    import torch

    layout, xf, xi = fc.build_inputs(recipe)
    k = recipe["k"]
    payloads = fc.state_dicts(layout, xf, xi)
    entries, nf, ni = layout_of(payloads[0])
    assert (nf, ni) == (layout.n_f32, layout.n_i64)
    spy = _TorchSpy(torch)
    aggregations.torch = spy
    try:
        result = aggregations.get()(None, None, payloads)
    finally:
        aggregations.torch = torch
    assert list(result) == list(payloads[0])
    names = [c[0] for c in spy.calls]
    assert names == ["mean"] + ["dot", "norm", "norm"] * k + ["maximum", "sum"] + ["norm", "norm"] * k + ["sum"], names
    vals = [c[2] for c in spy.calls]
    f32 = lambda t: np.float32(t.item())  # noqa: E731
    mean_flat = vals[0].numpy()
    dots = [f32(vals[1 + 3 * i]) for i in range(k)]
    nm = f32(vals[2])
    norms = [f32(vals[3 + 3 * i]) for i in range(k)]
    assert all(f32(vals[2 + 3 * i]) == nm for i in range(k))
    at = 1 + 3 * k
    cos, clipped, total = spy.calls[at][1].numpy(), vals[at].numpy(), vals[at + 1]
    norms_eps = [f32(vals[at + 2 + 2 * i]) for i in range(k)]
    weights = (vals[at] / (total + 1e-9)).numpy()  # aggregations.py:427, on the reference's own values
    n_clipped = int(np.sum(cos < 0))
    assert n_clipped >= len(recipe["negate"]), (recipe["name"], n_clipped)
    recipe["clipped_clients"] = n_clipped

    cols = fo.columns(xf, xi)
    mean_ref = np.empty(nf + ni, dtype=np.float32)
    mean_ref[region_index(entries, nf)] = mean_flat
    cos_ref64 = fo.cosine64(cols, mean_ref)
    cos_seq64 = fo.cosine64(cols, fo.mean(xf, xi))
    ref_self_err = np.abs(cos.astype(np.float64) - cos_ref64)
    mean_order_shift = np.abs(cos_seq64 - cos_ref64)

    out_f, out_i, dtypes = fc.flat_result(layout, result)
    cf, ci = canon(out_f), canon(out_i)
    sf, si = fc.sample_index(cf.size), fc.sample_index(ci.size)
    if recipe["model"] == "lenet5" and k in fc.FULL_KS:
        full[recipe["name"] + ".f32"] = cf
    hx = lambda seq: [f32hex(v) for v in seq]  # noqa: E731
    return {"recipe": recipe,
            "expected": {"nm": f32hex(nm), "dots": hx(dots), "norms": hx(norms), "norms_eps": hx(norms_eps),
                         "cos": hx(cos), "clipped": hx(clipped), "sum_clipped": f32hex(f32(total)),
                         "weights": hx(weights),
                         "ref_self_err": [float(v) for v in ref_self_err],
                         "mean_order_shift": [float(v) for v in mean_order_shift],
                         "sha_f32": sha(cf), "sha_i64f": sha(ci), "dtypes": dtypes,
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

        server = dict(Config().server._asdict(), secure_aggregation_type="Fl-trust")
        Config.server = types.SimpleNamespace(**server)
        import aggregations

        full, cases = {}, []
        for recipe in fc.recipes():
            cases.append(run_case(recipe, aggregations, full))
            exp = cases[-1]["expected"]
            print(recipe["name"], "clipped", recipe["clipped_clients"], "self err %.2e" % max(exp["ref_self_err"]),
                  "order shift %.2e" % max(exp["mean_order_shift"]), flush=True)
    with open(os.path.join(HERE, "fltrust_cases.json"), "w") as f:
        json.dump({"reference": "examples/detector/aggregations.py: fl_trust", "cases": cases}, f, indent=0)
    np.savez(os.path.join(HERE, "fltrust_full_small.npz"), **full)


if __name__ == "__main__":
    main()
