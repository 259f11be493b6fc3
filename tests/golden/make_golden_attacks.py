"""Generate the attack fixtures from the reference (TL-System/plato, examples/detector).

    python tests/golden/make_golden_attacks.py --reference /path/to/plato

Runs ``attacks.get()`` of examples/detector/attacks.py with ``Config().clients.attack_type`` set to "LIE",
"Lambda_attack", "Min-Max" and "Min-Sum" on the inputs of tests/attack_cases.build_inputs, called as the
detector server calls it: ``attack(baseline_weights, attacker_weights, deltas_received, num_attackers)``.
Writes

    tests/golden/attack_cases.json        recipe, digests of every poisoned payload, digests and samples of
                                          the poison and of the vector it came from, z, and for the searches
                                          the reference's lambda, norm and threshold and the float64 interval
    tests/golden/attack_full_small.npz    the whole vector of a few small cases

What the reference formed on the way is read off its own calls: a spy in place of its ``torch`` module
records the results of mean, std, norm, max, min and sum, and its ``perform_model_poisoning`` is wrapped to
record the poison.  The reference keeps its lambda in a local; it is recovered by replaying the halving
search (plato_amd.attacks.halving_search) on the recorded outcomes of its own comparisons, and checked:
the replayed lambda times the recorded unit vector must be the recorded poison, bit for bit.

Asserted for every case:
    - plato_amd.attacks.lie_z has the float64 bits of the reference's scipy.stats.norm.cdf value;
    - tests/attack_oracle.add_scaled_rows of the reference's own vector and scalar gives its poisoned
      payloads bit for bit (the restatement of perform_model_poisoning, counters included);
    - the oracle std is the reference's, bit for bit; the oracle mean is, up to A = 4;
    - the reference's lambda lies in [lambda_lo, lambda_hi]: the results of the same search with the
      predicate in float64 from the fp32 differences against the thresholds T (1 -+ 2 eps), T the float64
      threshold and eps = (PLATO_AGG_PAIRDIST_CHAIN + 1) * 2^-24.  A seed where it does not is replaced.
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

from make_golden import boot_reference, f32hex, layout_of  # noqa: E402
from make_golden_fltrust import region_index  # noqa: E402

from plato_amd import attacks as host  # noqa: E402
from tests import attack_cases as ac  # noqa: E402
from tests import attack_oracle as ao  # noqa: E402
from tests import krum_oracle as ko  # noqa: E402

RECORDED = ("mean", "std", "norm", "max", "min", "sum")


class _TorchSpy:
    """The torch module with the results of the reductions recorded: (name, number of tensors, result)."""

    def __init__(self, torch):
        self._torch, self.calls = torch, []

    def __getattr__(self, name):
        fn = getattr(self._torch, name)
        if name not in RECORDED:
            return fn

        def recorded(*args, **kwargs):
            out = fn(*args, **kwargs)
            tensors = sum(isinstance(a, self._torch.Tensor) for a in args)
            self.calls.append((name, tensors, out.detach().clone()))
            return out

        return recorded


def arena_order(entries, nf, flat: np.ndarray) -> np.ndarray:
    """The reference's flat vector (state-dict order) in [fp32 region | int64 region] order."""
    out = np.empty(flat.size, dtype=np.float32)
    out[region_index(entries, nf)] = flat
    return out


def replay(outcomes, keep_failed):
    it = iter(outcomes)
    lam = host.halving_search(lambda _lam: next(it), keep_failed)
    assert next(it, None) is None, "the replayed search took fewer steps than the reference"
    return lam


def run_case(recipe, ref_attacks, full):
    import torch

    kind, a = recipe["kind"], recipe["a"]
    layout, bf, bi, wf, wi = ac.build_inputs(recipe)
    baseline = ac.state_dict(layout, bf, bi)
    payloads = [ac.state_dict(layout, wf[c], wi[c]) for c in range(a)]
    deltas = [type(p)((n, p[n] - baseline[n]) for n in p) for p in payloads]  # compute_weight_deltas
    entries, nf, ni = layout_of(payloads[0])
    assert (nf, ni) == (layout.n_f32, layout.n_i64)

    from plato.config import Config

    clients = dict(Config().clients._asdict() if hasattr(Config().clients, "_asdict") else vars(Config().clients))
    clients.update(attack_type=ac.ATTACK_TYPE[kind], per_round=recipe.get("per_round", 100),
                   lambada_value=recipe.get("lambada_value", ac.LAMBADA))
    Config.clients = types.SimpleNamespace(**clients)

    spy, poisons = _TorchSpy(torch), []
    poisoning = ref_attacks.perform_model_poisoning
    ref_attacks.torch = spy
    ref_attacks.perform_model_poisoning = lambda w, poison: (poisons.append(poison.detach().clone()), poisoning(w, poison))[1]
    try:
        result = ref_attacks.get()(baseline, payloads, deltas, a)
    finally:
        ref_attacks.torch, ref_attacks.perform_model_poisoning = torch, poisoning
    assert len(result) == a
    rows = [ac.flat_payload(layout, p) for p in result]
    exp = {"rows": [ac.row_digest(f, i) for f, i in rows]}
    if kind == "lie" and a == 1:
        assert not poisons and all(np.array_equal(rows[0][j], (wf, wi)[j][0]) for j in range(2))
        return {"recipe": recipe, "expected": exp}
    poison = arena_order(entries, nf, poisons[0].numpy())
    by_name = lambda name: [c for c in spy.calls if c[0] == name]  # noqa: E731

    d_f32 = (wf - bf[None, :]).astype(np.float32)
    d_i64 = wi - bi[None, :]
    u = ao.columns(d_f32, d_i64)
    if kind == "lie":
        vector = arena_order(entries, nf, by_name("std")[0][2].numpy())
        n = recipe["per_round"]
        from scipy.stats import norm as scipy_norm

        z = float(scipy_norm.cdf((n - (n / 2 + 1 - a)) / n))
        assert z == host.lie_z(n, a), (recipe["name"], z, host.lie_z(n, a))
        exp["z"] = z.hex()
        s = -np.float32(z)
        assert np.array_equal(ac.canon(ao.column_std(u)).view(np.uint32), ac.canon(vector).view(np.uint32))
    elif kind == "lambda":
        vector = arena_order(entries, nf, by_name("mean")[0][2].numpy())
        s = -np.float32(recipe["lambada_value"])
    else:
        minsum = kind == "minsum"
        vector = arena_order(entries, nf, by_name("mean")[0][2].numpy())
        norm = np.float32(by_name("norm")[0][2].item())
        p = ao.unit(vector, norm)
        if minsum:
            t_ref = by_name("min")[-1][2]
            last = max(j for j, c in enumerate(spy.calls) if c[0] == "min")
            scores = [c[2] for c in spy.calls[last + 1:] if c[0] == "sum"]
        else:
            pair = [j for j, c in enumerate(spy.calls) if c[0] == "max" and c[1] == 2]
            t_ref = spy.calls[pair[-1]][2]
            scores = [c[2] for c in spy.calls[pair[-1] + 1:] if c[0] == "max"]
        lam = replay([bool(sc <= t_ref) for sc in scores], minsum)
        s = ao.scalar_of(kind, lam)
        dist = ko.pairwise_sqdist(d_f32, d_i64)
        t64 = ao.threshold(kind, dist)
        lo = ao.search(kind, u, vector, p, t64 * (1 - 2 * ao.EPS_DIST))
        hi = ao.search(kind, u, vector, p, t64 * (1 + 2 * ao.EPS_DIST))
        mine = ao.search(kind, u, vector, p, t64)
        if not lo <= lam <= hi:
            return None  # another seed
        exp.update(lambda_ref=f32hex(lam), lambda_lo=f32hex(lo), lambda_hi=f32hex(hi), lambda_f64=f32hex(mine),
                   norm_ref=f32hex(norm), norm_f64=float(ao.norm64(vector)).hex(),
                   threshold_ref=f32hex(np.float32(t_ref.item())), threshold_f64=float(t64).hex(),
                   search_steps=len(scores))
    if kind != "lie" and a <= 4:
        cols = ao.columns(wf, wi) if kind == "minsum" else u
        assert np.array_equal(ao.mean(cols).view(np.uint32), vector.view(np.uint32)), recipe["name"]
    # the restatement of perform_model_poisoning on the reference's own vector and scalar
    with np.errstate(invalid="ignore", over="ignore"):
        v = p if kind in ("minmax", "minsum") else vector
        assert np.array_equal(ac.canon((np.float32(s) * v).astype(np.float32)).view(np.uint32),
                              ac.canon(poison).view(np.uint32)), recipe["name"]
    out_f, out_i = ao.add_scaled_rows(wf, wi, s, v)
    assert [ac.row_digest(out_f[c], out_i[c]) for c in range(a)] == exp["rows"], recipe["name"]
    exp.update(s=f32hex(s), sha_poison=ac.sha(ac.canon(poison)), samples_poison=ac.samples(poison),
               sha_vector=ac.sha(ac.canon(vector)), samples_vector=ac.samples(vector),
               samples_row0=ac.samples(np.concatenate([rows[0][0], rows[0][1].astype(np.float32)])))
    if recipe["name"] in ac.FULL or recipe["model"] == "bn_toy":
        full[recipe["name"] + ".vector"] = vector
    return {"recipe": recipe, "expected": exp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        boot_reference(args.reference, work)
        sys.path.insert(0, os.path.join(args.reference, "examples/detector"))
        import attacks as ref_attacks

        full, cases = {}, []
        for recipe in ac.recipes():
            for attempt in range(8):
                case = run_case(dict(recipe, seed=recipe["seed"] + 1000 * attempt), ref_attacks, full)
                if case is not None:
                    break
            else:
                raise AssertionError(f"{recipe['name']}: no seed puts the reference's lambda in the interval")
            cases.append(case)
            e = case["expected"]
            print(recipe["name"], "seed", case["recipe"]["seed"],
                  *(f"{k}={e[k]}" for k in ("lambda_ref", "lambda_lo", "lambda_hi", "search_steps") if k in e), flush=True)
    with open(os.path.join(HERE, "attack_cases.json"), "w") as f:
        json.dump({"reference": "examples/detector/attacks.py: lie_attack, lambda_attack, min_max_attack, "
                                "min_sum_attack", "cases": cases}, f, indent=0)
    np.savez(os.path.join(HERE, "attack_full_small.npz"), **full)


if __name__ == "__main__":
    main()
