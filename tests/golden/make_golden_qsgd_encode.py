"""Generate the QSGD-quantizer fixtures from the reference (TL-System/plato).

    python tests/golden/make_golden_qsgd_encode.py --reference /path/to/plato

Runs ``plato.processors.model_quantize_qsgd.Processor._process_layer`` on the CPU over every entry of the
cases of tests/qsgd_encode_cases.py.  The reference seeds Python's ``random`` from the OS and draws one
``random.random()`` per element; here ``random.seed`` does nothing and ``random.random`` hands out the
project's draws (tests/qsgd_encode_oracle.py: ``draws``) for the row elements the entry occupies when the
state is staged entry after entry into one row.  Everything else is the reference's own arithmetic and byte
packing.  It is never needed at test time.  Writes

    tests/golden/qsgd_encode_cases.json   per case: level, draw seed, the entries (name, dtype, shape) in
                                          order, the torch and numpy versions
    tests/golden/qsgd_encode_small.npz    ``<case>/in/<key>`` the entry as raw bits (uint32, or int64) and
                                          ``<case>/out/<key>`` the bytes the reference returned

Asserted for every entry: the reference consumed exactly numel draws, and tests/qsgd_encode_oracle.py gives
the same bytes.
"""

from __future__ import annotations

import argparse
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import boot_reference  # noqa: E402

from tests import qsgd_encode_cases as qc  # noqa: E402
from tests import qsgd_encode_oracle as qo  # noqa: E402


class Feed:
    """Stands in for ``random.random`` and ``random.seed`` while one entry is quantized."""

    def __init__(self, u: np.ndarray):
        self.values = [float(x) for x in u]
        self.taken = 0

    def random(self) -> float:
        self.taken += 1
        return self.values[self.taken - 1]

    def seed(self, *args, **kwargs) -> None:
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    boot_reference(args.reference, tempfile.mkdtemp(prefix="qsgd_encode_golden_"))
    import torch
    from plato.processors import model_quantize_qsgd

    arrays, out_cases = {}, []
    for recipe in qc.recipes():
        st = qc.seeded_state(recipe)
        proc = model_quantize_qsgd.Processor(quantization_level=recipe["level"], server_id=0)
        expected = qo.encode_state(st, recipe["level"], recipe["draw_seed"])
        entries, at = [], 0
        for key, a in st.items():
            tensor = torch.from_numpy(np.array(a))
            feed = Feed(qo.draws(recipe["draw_seed"], at, a.size))
            keep = random.random, random.seed
            random.random, random.seed = feed.random, feed.seed
            try:
                blob = proc._process_layer(tensor)
            finally:
                random.random, random.seed = keep
            assert feed.taken == a.size, (recipe["name"], key, "draws taken", feed.taken)
            assert blob == expected[key], (recipe["name"], key, "the oracle differs from the reference")
            flat = np.ascontiguousarray(a).reshape(-1)
            arrays[f"{recipe['name']}/in/{key}"] = flat.view(np.uint32).copy() if a.dtype == np.float32 else flat.copy()
            arrays[f"{recipe['name']}/out/{key}"] = np.frombuffer(blob, dtype=np.uint8).copy()
            entries.append([key, str(a.dtype), list(a.shape)])
            at += a.size
        out_cases.append({"name": recipe["name"], "state": recipe["state"], "seed": recipe["seed"],
                          "level": recipe["level"], "draw_seed": recipe["draw_seed"], "numel": at, "entries": entries})
        print(f"{recipe['name']:14s} level={recipe['level']:3d} entries={len(entries):3d} numel={at}")
    meta = {"torch": torch.__version__, "numpy": np.__version__, "cases": out_cases}
    with open(qc.JSON_PATH, "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    np.savez_compressed(qc.NPZ_PATH, **arrays)
    print("wrote", qc.JSON_PATH, os.path.getsize(qc.NPZ_PATH), "bytes of npz")


if __name__ == "__main__":
    main()
