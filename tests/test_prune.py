"""Global magnitude pruning without a GPU: the numpy restatement (tests/prune_oracle.py) against the
reference fixtures (tests/golden/prune_*), bit for bit; the reference's count k and its errors; the key
order the host layer leaves behind; the host-side refusals of plato_agg_prune_global; and the drop-in's
refusal of other pruning methods."""

import os

import numpy as np
import pytest
import torch
import torch.nn.utils.prune as torch_prune

from plato_amd import _lib
from plato_amd import prune as host
from plato_amd.processors import UnstructuredPruning
from plato_amd.processors.prune import Processor
from tests import prune_cases as pc
from tests import prune_oracle as po

built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")


def test_the_fixture_covers_every_recipe():
    assert [c["name"] for c in pc.cases()] == pc.case_ids()
    for c, r in zip(pc.cases(), pc.recipes()):
        assert (c["model"], c["amount"], c["applications"]) == (r["model"], r["amount"], r["applications"])
        assert len(c["keys_out"]) == len(c["records"]) == c["applications"]


@pytest.mark.parametrize("name", pc.case_ids())
def test_oracle_equals_the_reference_bit_for_bit(name):
    c = pc.case(name)
    model = pc.build(c["model"])
    names = pc.prunable_names(model)
    assert names == c["prunable"]
    module_names = {m: n for n, m in model.named_modules()}
    assert [f"{module_names[m]}.{p}" for m, p in host.prunable_weights(model)] == names
    before = pc.state_bits(c, "in")
    n = sum(before[k].size for k in names)
    assert n == c["n"] and host.nparams_toprune(pc.amount_of(c), n) == c["k"]
    for a in range(1, c["applications"] + 1):
        after = pc.state_bits(c, f"out{a}")
        row, pieces, where = pc.as_row(before, names)
        got, record = po.prune_row(row, pieces, c["k"])
        for key, (b, e) in where.items():  # every entry, the untouched ones included, nothing canonicalised
            assert got[b:e].tobytes() == after[key].view(np.uint32).tobytes(), (name, a, key)
        assert dict(zip(("T", "below", "ties", "r"), record)) == c["records"][a - 1]
        assert int(np.count_nonzero(got != row)) <= c["k"]
        before = after


@pytest.mark.parametrize("name", ["toy_float", "toy_zero_int", "resblock_half", "toy_thrice"])
def test_key_order_after_each_application(name):
    """prune.remove re-registers the weight last: bias before weight from the first application on, also
    when k = 0.  The re-registration is the host layer's alone, so it is checked here with the device step
    left out (k = 0 launches nothing)."""
    c = pc.case(name)
    model = pc.load_model(c)
    assert list(model.state_dict()) == c["keys_in"]
    for a in range(c["applications"]):
        host.prune_model(model, 0, device="cpu")
        assert list(model.state_dict()) == c["keys_out"][a]
    assert {k: v.tobytes() for k, v in pc.model_bits(model).items()} == \
        {k: v.tobytes() for k, v in pc.state_bits(c, "in").items()}


def test_nparams_toprune_is_the_reference_count():
    for amount, n in [(0.2, 252), (0.125, 252), (0.375, 252), (0.5, 491), (0.5, 5), (0.5, 7), (1.0, 9), (0.0, 9),
                      (0, 9), (9, 9), (3, 9), (0.3, 11_166_912), (0.8, 11_166_912), (True, 4), (np.float32(0.25), 10),
                      (np.int64(3), 10)]:
        assert host.nparams_toprune(amount, n) == torch_prune._compute_nparams_toprune(amount, n), (amount, n)
    assert host.nparams_toprune(0.125, 252) == 32 and host.nparams_toprune(0.375, 252) == 94  # round half to even


@pytest.mark.parametrize("amount, n", [(-1, 10), (-0.1, 10), (1.5, 10), (11, 10), (np.int64(-2), 5)])
def test_the_reference_value_errors(amount, n):
    """The same conditions as torch's two checks (their wording belongs to the torch version)."""
    with pytest.raises(ValueError, match=f"amount={amount} should"):
        host.nparams_toprune(amount, n)
    with pytest.raises(ValueError, match=f"amount={amount} should"):
        torch_prune._validate_pruning_amount_init(amount)
        torch_prune._validate_pruning_amount(torch_prune._compute_nparams_toprune(amount, n), n)


def test_amount_type_error():
    with pytest.raises(TypeError):
        host.nparams_toprune("0.2", 10)
    with pytest.raises(TypeError):
        torch_prune._validate_pruning_amount_init("0.2")


def _table(*pieces):
    return host.piece_table(list(pieces))


@built
def test_prune_global_argument_errors_are_raised_without_gpu_work():
    """Every call below fails a check, or has nothing to do, before any launch or copy."""
    a = 1 << 12  # any 256-byte-aligned non-null address: nothing is dereferenced on these paths
    lib = _lib.lib()

    def call(row, n_row, table, k, ws=a, res=a):
        _lib.call("plato_agg_prune_global", row, n_row, table.ctypes.data if len(table) else None, len(table), k,
                  ws, res, None)

    with pytest.raises(ValueError, match="ends before it begins"):
        call(a, 100, _table((0, 10), (30, 20)), 1)
    with pytest.raises(ValueError, match="overlap or are out of order"):
        call(a, 100, _table((0, 10), (9, 20)), 1)
    with pytest.raises(ValueError, match="overlap or are out of order"):
        call(a, 100, _table((50, 60), (0, 10)), 1)
    with pytest.raises(ValueError, match="past the row"):
        call(a, 100, _table((0, 10), (90, 101)), 1)
    with pytest.raises(ValueError, match="k exceeds"):
        call(a, 100, _table((0, 10), (10, 20)), 21)
    with pytest.raises(ValueError, match="k exceeds"):
        call(a, 100, _table(), 1)
    with pytest.raises(ValueError, match="2\\^32"):
        call(a, 1 << 32, _table((0, 10)), 1)
    with pytest.raises(ValueError, match="2\\^20 pieces"):
        _lib.call("plato_agg_prune_global", a, 100, a, (1 << 20) + 1, 1, a, a, None)
    with pytest.raises(ValueError, match="null piece table"):
        _lib.call("plato_agg_prune_global", a, 100, None, 2, 1, a, a, None)
    with pytest.raises(ValueError, match="null row"):
        call(None, 100, _table((0, 10)), 1)
    with pytest.raises(ValueError, match="null row"):
        call(a, 100, _table((0, 10)), 1, ws=None)
    with pytest.raises(ValueError, match="null row"):
        call(a, 100, _table((0, 10)), 1, res=None)
    with pytest.raises(ValueError, match="row must be 16-byte aligned"):
        call(a + 4, 100, _table((0, 10)), 1)
    with pytest.raises(ValueError, match="workspace must be 256-byte aligned"):
        call(a, 100, _table((0, 10)), 1, ws=a + 128)
    with pytest.raises(ValueError, match="result must be 16-byte aligned"):
        call(a, 100, _table((0, 10)), 1, res=a + 8)
    # k = 0: a success with nothing launched or written, whatever the pointers; the table is still checked
    assert lib.plato_agg_prune_global(None, 100, _table((3, 10), (10, 10)).ctypes.data, 2, 0, None, None, None) == 0
    assert lib.plato_agg_prune_global(None, 0, None, 0, 0, None, None, None) == 0
    with pytest.raises(ValueError, match="ends before it begins"):
        call(a, 100, _table((5, 4)), 0)
    # the workspace: 0 for counts the 32-bit counters and tables do not hold
    assert lib.plato_agg_prune_global_workspace((1 << 20) + 1, 10) == 0
    assert lib.plato_agg_prune_global_workspace(1, 1 << 32) == 0
    small, large = lib.plato_agg_prune_global_workspace(1, 1), lib.plato_agg_prune_global_workspace(21, 11_166_912)
    assert small % 256 == 0 and small >= 256 + 3 * 2048 * 4 and large > small


def test_host_layer_refuses_before_the_device():
    with pytest.raises(ValueError, match="contiguous 1-d float32"):
        host.prune_row(torch.zeros(8, dtype=torch.float64), [(0, 8)], 1)
    with pytest.raises(RuntimeError, match="no host path"):
        host.prune_row(torch.zeros(8), [(0, 8)], 1)
    with pytest.raises(ValueError, match="outside a row"):
        host.piece_table([(0, 1 << 32)])
    model = pc.build("toy")
    with pytest.raises(ValueError, match="should be smaller than the number of parameters"):
        host.prune_model(model, 253, device="cpu")
    with pytest.raises(ValueError, match="float in the range"):
        host.prune_model(model, 1.5, device="cpu")
    assert list(model.state_dict())[:2] == ["0.weight", "0.bias"]  # a refused call re-registers nothing


def test_drop_in_constructor_and_refusals():
    assert UnstructuredPruning is Processor
    p = Processor(name="unstructured_pruning", trainer=object(), server_id=3)
    assert (p.parameters_to_prune, p.pruning_method, p.amount) == (None, torch_prune.L1Unstructured, 0.2)
    assert (p.name, p.client_id, p.server_id) == ("unstructured_pruning", None, 3) and repr(p) == "unstructured_pruning"
    for method in (torch_prune.RandomUnstructured, torch_prune.LnStructured, torch_prune.Identity):
        with pytest.raises(NotImplementedError, match="L1Unstructured"):
            Processor(pruning_method=method)


def test_drop_in_with_nothing_to_prune_needs_no_device():
    """amount = 0 changes no bit, re-registers the weights and returns the CPU state dict; ``data`` is ignored."""
    c = pc.case("toy_zero_int")

    class Trainer:
        model = pc.load_model(c)

    p = Processor(amount=0, trainer=Trainer(), server_id=0)
    out = p.process("ignored")
    assert list(out) == c["keys_out"][0] and p.model is Trainer.model
    exp = pc.state_bits(c, "out1")
    for key, t in out.items():
        assert t.numpy().reshape(-1).view(np.uint32 if t.dtype == torch.float32 else np.int64).tobytes() == \
            exp[key].tobytes()
    assert p.last_result.k == 0
