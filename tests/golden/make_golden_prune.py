"""Generate the pruning fixtures from the reference (TL-System/plato).

    python tests/golden/make_golden_prune.py --reference /path/to/plato

Runs ``plato.processors.unstructured_pruning.Processor`` on the CPU over the cases of tests/prune_cases.py:
the model is built, its state is drawn from the case's seed (numpy's PCG64, scaled normal weights) and
edited as the case asks, and ``process`` is applied the case's number of times to the same model, as the
server's outbound pipeline does.  It is never needed at test time.  Writes

    tests/golden/prune_cases.json     per case: model, amount and its type, n, k, the ``state_dict()`` key
                                      order before and after every application, the threshold key and the
                                      tie counts of every application, the torch and numpy versions
    tests/golden/prune_full_small.npz the state before and after every application as raw bits
                                      (``<case>/in/<key>``, ``<case>/out<a>/<key>``)

Asserted for every application: the reference's answer is the only possible one, that is the sorted keys
``bits & 0x7fffffff`` at ranks k - 1 and k differ, or every element tied there is +-0, or k is 0 or n; the
reference pruned exactly the elements tests/prune_oracle.py prunes, to the same bits; and k is
``plato_amd.prune.nparams_toprune``.  A case whose seed fails the first is given another seed by hand.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import boot_reference  # noqa: E402

from plato_amd import prune as host  # noqa: E402
from tests import prune_cases as pc  # noqa: E402
from tests import prune_oracle as po  # noqa: E402

QNANS = [0x7FC00001, 0xFFC12345, 0x7FE00000]   # quiet, distinct keys
SNANS = [0x7F800001, 0xFFA00000]               # signalling: only where they are pruned
INFS = [0x7F800000, 0xFF800000]


def edit_zeros(flat, rng):
    at = rng.choice(flat.size, 100, replace=False)
    flat[at] = np.where(np.arange(100) % 2 == 0, np.uint32(0), np.uint32(0x80000000))


def edit_nonfinite(flat, rng, signalling=False):
    values = INFS + QNANS + (SNANS if signalling else [])
    at = rng.choice(flat.size, len(values), replace=False)
    flat[at] = np.array(values, dtype=np.uint32)


def edit_subnormals(flat, rng):
    at = rng.choice(flat.size, 32, replace=False)
    flat[at[:20]] = np.where(np.arange(20) % 3 == 0, np.uint32(0x80000000), np.uint32(0))
    mant = rng.choice(np.arange(1, 1 << 23), 12, replace=False).astype(np.uint32)  # distinct subnormals
    flat[at[20:]] = mant | np.where(np.arange(12) % 2 == 0, np.uint32(0x80000000), np.uint32(0))


EDITS = {None: lambda flat, rng: None, "zeros": edit_zeros, "nonfinite": edit_nonfinite,
         "nonfinite_snan": lambda flat, rng: edit_nonfinite(flat, rng, True), "subnormals": edit_subnormals}


def seeded_model(recipe):
    import torch

    rng = np.random.default_rng(recipe["seed"])
    model = pc.build(recipe["model"])
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if t.dtype == torch.float32:
                scale = 1.0 if "running_var" in key else 0.1
                a = (rng.standard_normal(t.numel()) * scale).astype(np.float32)
                if "running_var" in key:
                    a = np.abs(a) + np.float32(0.5)
                t.copy_(torch.from_numpy(a).reshape(t.shape))
            else:
                t.fill_(int(rng.integers(1, 1000)))
        names = pc.prunable_names(model)
        sd = model.state_dict()
        flat = np.concatenate([sd[k].numpy().reshape(-1).view(np.uint32) for k in names])
        EDITS[recipe["edit"]](flat, rng)
        at = 0
        for k in names:
            n = sd[k].numel()
            sd[k].copy_(torch.from_numpy(flat[at:at + n].view(np.float32).copy()).reshape(sd[k].shape))
            at += n
    return model


def unique_answer(keys_sorted, k):
    n = keys_sorted.size
    return k in (0, n) or keys_sorted[k - 1] != keys_sorted[k] or keys_sorted[k - 1] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    boot_reference(args.reference, tempfile.mkdtemp(prefix="prune_golden_"))
    import torch
    from plato.processors import unstructured_pruning

    class Trainer:
        model = None

    arrays, out_cases = {}, []
    for recipe in pc.recipes():
        model = seeded_model(recipe)
        names = pc.prunable_names(model)
        trainer = Trainer()
        trainer.model = model
        proc = unstructured_pruning.Processor(amount=recipe["amount"], name="unstructured_pruning", trainer=trainer,
                                              server_id=0)
        before = pc.model_bits(model)
        for key, a in before.items():
            arrays[f"{recipe['name']}/in/{key}"] = a
        n = int(sum(before[k].size for k in names))
        k = host.nparams_toprune(recipe["amount"], n)
        record = {"name": recipe["name"], "model": recipe["model"], "seed": recipe["seed"], "edit": recipe["edit"],
                  "amount": recipe["amount"], "amount_type": "int" if isinstance(recipe["amount"], int) else "float",
                  "applications": recipe["applications"], "n": n, "k": k, "prunable": names,
                  "keys_in": list(before), "keys_out": [], "records": []}
        for a in range(1, recipe["applications"] + 1):
            flat = np.concatenate([before[key] for key in names])
            assert unique_answer(np.sort(po.keys(flat)), k), (recipe["name"], a, "the reference's answer is not unique")
            returned = proc.process(None)
            after = pc.model_bits(model)
            assert list(returned) == list(after)
            got = np.concatenate([after[key] for key in names])
            exp, rec = po.prune_flat(flat, k)
            assert got.tobytes() == exp.tobytes(), (recipe["name"], a, "the oracle differs from the reference")
            assert int(np.count_nonzero(got != flat)) <= k
            for key in after:
                if key not in names:
                    assert after[key].tobytes() == before[key].tobytes(), (recipe["name"], key)
                arrays[f"{recipe['name']}/out{a}/{key}"] = after[key]
            record["keys_out"].append(list(after))
            record["records"].append({"T": rec[0], "below": rec[1], "ties": rec[2], "r": rec[3]})
            before = after
        out_cases.append(record)
        print(f"{recipe['name']:28s} n={n:6d} k={k:6d} T={record['records'][0]['T']:#010x} keys_out={record['keys_out'][0][:3]}")
    meta = {"torch": torch.__version__, "numpy": np.__version__, "cases": out_cases}
    with open(pc.JSON_PATH, "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    np.savez_compressed(pc.NPZ_PATH, **arrays)
    print("wrote", pc.JSON_PATH, os.path.getsize(pc.NPZ_PATH), "bytes of npz")


if __name__ == "__main__":
    main()
