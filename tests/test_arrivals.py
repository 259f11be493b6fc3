"""Arrival staging without a device: the table every engine kind keeps (which payload owns which slot,
whether a staged copy is still the payload's) and the rule by which a round adopts a staged row."""

import itertools
from collections import OrderedDict

import pytest
import torch

from plato_amd.arrivals import Adopt, ArrivalTable, adopt_rule, adopt_or_put

CHUNK = 16
SIG = ("layout", 1)


def _payload(seed=0):
    g = torch.Generator().manual_seed(seed)
    return OrderedDict(w=torch.randn(5, generator=g), n=torch.tensor(3))


class _Slabs:
    """An engine's side of ``take``: every ``grow`` is one more slab of CHUNK slots."""

    def __init__(self):
        self.grown = 0

    def grow(self):
        self.grown += 1
        return [(self.grown, r) for r in range(CHUNK)]


def _stage(table, slabs, payload, codec="native", signature=SIG, delta_key=None):
    slot = table.take(codec, slabs.grow)
    table.file(payload, codec, signature, ("rows of", slot), slot, delta_key)
    return table[id(payload)]


# ------------------------------------------------------------------ lookup
def test_lookup_returns_the_record_of_the_same_object_only():
    table, slabs = ArrivalTable(), _Slabs()
    p = _payload()
    rec = _stage(table, slabs, p, delta_key="K1")
    assert table.lookup(p, "native", SIG) is rec
    assert (rec.payload, rec.codec, rec.signature, rec.delta_key) == (p, "native", SIG, "K1")
    assert rec.rows == ("rows of", rec.slot)
    same_tensors = OrderedDict(p)  # an equal dict (the very same tensors), another object
    assert same_tensors == p and table.lookup(same_tensors, "native", SIG) is None
    assert table.lookup(p, "bf16", SIG) is None
    assert table.lookup(p, "native", ("layout", 2)) is None
    assert table.lookup(p, "native", SIG) is rec  # the refusals changed nothing


def test_lookup_refuses_a_payload_edited_after_it_was_filed():
    table, slabs = ArrivalTable(), _Slabs()
    replaced, written = _payload(1), _payload(2)
    _stage(table, slabs, replaced)
    _stage(table, slabs, written)
    replaced["w"] = replaced["w"] + 1.0
    written["w"].add_(1.0)
    assert table.lookup(replaced, "native", SIG) is None
    assert table.lookup(written, "native", SIG) is None


def test_lookup_ignores_a_record_moved_under_another_objects_id():
    table, slabs = ArrivalTable(), _Slabs()
    p, other = _payload(), _payload()
    rec = _stage(table, slabs, p)
    table[id(other)] = table.pop(id(p))  # what a recycled id() would look like
    assert table.lookup(other, "native", SIG) is None
    assert table.lookup(p, "native", SIG) is None
    assert table[id(other)] is rec


# ------------------------------------------------------------------- slots
def test_slots_grow_by_slabs_and_come_back_once():
    table, slabs = ArrivalTable(), _Slabs()
    pays = [_payload(i) for i in range(2 * CHUNK + 1)]
    for p in pays[:CHUNK]:
        _stage(table, slabs, p)
    assert slabs.grown == 1 and table.free_count() == 0
    _stage(table, slabs, pays[CHUNK])
    assert slabs.grown == 2 and table.free_count() == CHUNK - 1
    assert len(table) == CHUNK + 1
    table.release()
    assert table == {}
    assert table.free_count() == 2 * CHUNK
    assert len(set(table.free["native"])) == 2 * CHUNK  # no slot twice
    table.release()
    assert table.free_count() == 2 * CHUNK  # nothing left to return
    for p in pays[:CHUNK + 1]:
        _stage(table, slabs, p)
    assert slabs.grown == 2  # the freed slots serve the next arrivals
    assert table.free_count() == CHUNK - 1


def test_free_lists_are_per_codec():
    table, slabs = ArrivalTable(), _Slabs()
    _stage(table, slabs, _payload(0), codec="native")
    _stage(table, slabs, _payload(1), codec="bf16")
    assert slabs.grown == 2
    assert {c: len(v) for c, v in table.free.items()} == {"native": CHUNK - 1, "bf16": CHUNK - 1}


def test_drop_returns_exactly_that_payloads_slot():
    table, slabs = ArrivalTable(), _Slabs()
    a, b, unknown = _payload(0), _payload(1), _payload(2)
    rec_a, rec_b = _stage(table, slabs, a), _stage(table, slabs, b)
    free = list(table.free["native"])
    table.drop(unknown)
    assert table.free["native"] == free and len(table) == 2
    table.drop(a)
    assert table.free["native"] == free + [rec_a.slot]
    assert id(a) not in table and table[id(b)] is rec_b
    # another object at b's id: b's record stays and nothing is freed
    table[id(unknown)] = table.pop(id(b))
    table.drop(unknown)
    assert table[id(unknown)] is rec_b
    assert table.free["native"] == free + [rec_a.slot]


def test_a_record_without_a_slot_frees_nothing():
    table = ArrivalTable()
    p = _payload()
    table.file(p, None, None, ["sub-payloads"])  # the entry-sharded engine's: its shards hold the slots
    rec = table.lookup(p, None, None)
    assert rec is table[id(p)] and rec.slot is None and rec.rows == ["sub-payloads"]
    table.release()
    assert table == {} and table.free_count() == 0


def test_reset_forgets_records_free_lists_and_the_baseline_key():
    table, slabs = ArrivalTable(), _Slabs()
    _stage(table, slabs, _payload())
    table.base_key = "K1"
    table.reset()
    assert table == {} and table.free == {} and table.base_key is None
    assert table.free_count() == 0
    _stage(table, slabs, _payload())
    assert slabs.grown == 2  # the old slab's slots are gone with the layout


# -------------------------------------------------------------------- rule
def _expected(delta_key, holds_deltas, has_baseline, base_key, same_bits):
    """The parent's ``AggregationRound.adopt`` / ``MultiRound.adopt``, as outcomes.

    Weights (no delta key) are always adopted: a delta round converts the row in place (and raises there
    if it has no baseline), a weight round uses it as it is.  A delta row is adopted only by a delta round
    whose staged baseline has the arrival baseline's key and, compared on the device, its bits.  The two
    rounds differed in one combination no round can be in, a baseline key without a staged baseline (the
    key is set by ``put_baseline`` only): the bucket round refused it by its ``has_baseline`` test, and
    that is what a round without a baseline to compare must do.
    """
    if delta_key is None:
        return Adopt.CONVERT
    if not holds_deltas or not has_baseline or delta_key != base_key:
        return Adopt.REFUSE
    return Adopt.AS_FORMED if same_bits else Adopt.REFUSE


@pytest.mark.parametrize("delta_key,holds_deltas,has_baseline,base_key,same_bits",
                         list(itertools.product([None, "K1"], [True, False], [True, False], ["K1", "K2"],
                                                [True, False])))
def test_adopt_rule(delta_key, holds_deltas, has_baseline, base_key, same_bits):
    calls = []

    def compare():
        calls.append(1)
        return same_bits

    got = adopt_rule(delta_key, holds_deltas, has_baseline, base_key, compare)
    assert got is _expected(delta_key, holds_deltas, has_baseline, base_key, same_bits)
    keys_match = delta_key is not None and holds_deltas and has_baseline and delta_key == base_key
    assert len(calls) == (1 if keys_match else 0)  # the device compare runs only when the keys match


def test_adopt_rule_outcomes_spelled_out():
    """The three outcomes at the cases the golden GPU test names (weights, deltas, deltas_stale,
    deltas_data_write), so a change to ``_expected`` and the rule together cannot pass unnoticed."""
    yes, no = (lambda: True), (lambda: False)
    assert adopt_rule(None, False, True, "K1", no) is Adopt.CONVERT      # weights into a weight round
    assert adopt_rule(None, True, True, "K1", no) is Adopt.CONVERT       # weights into a delta round
    assert adopt_rule("K1", True, True, "K1", yes) is Adopt.AS_FORMED    # deltas
    assert adopt_rule("K1", True, True, "K2", yes) is Adopt.REFUSE       # deltas_stale
    assert adopt_rule("K1", True, True, "K1", no) is Adopt.REFUSE        # deltas_data_write
    assert adopt_rule("K1", False, True, "K1", yes) is Adopt.REFUSE      # a delta row into a weight round
    assert adopt_rule("K1", True, False, None, yes) is Adopt.REFUSE      # no baseline staged yet


# ----------------------------------------------------------------- staging
def test_adopt_or_put_adopts_else_puts_in_slot_order():
    class Round:
        def __init__(self):
            self.calls = []

        def adopt(self, slot, payload):
            self.calls.append(("adopt", slot, payload))
            return payload == "staged"

        def put_client(self, slot, payload, *what):
            self.calls.append(("put", slot, payload, *what))

    rnd = Round()
    adopt_or_put(rnd, ["staged", "fresh", "staged"])
    assert rnd.calls == [("adopt", 0, "staged"), ("adopt", 1, "fresh"), ("put", 1, "fresh"), ("adopt", 2, "staged")]
    rnd = Round()
    adopt_or_put(rnd, ["fresh"], what="deltas_received")
    assert rnd.calls == [("adopt", 0, "fresh"), ("put", 0, "fresh", "deltas_received")]
