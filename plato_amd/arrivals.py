"""Arrival staging: the bookkeeping every engine kind shares, and the rule for adopting a staged row.

An engine's ``prestage`` copies a payload to HBM when it arrives, the next round adopts the staged row by
identity, and ``release_arrivals`` returns the slot.  What a row is (device pointers, per-shard rows,
sub-payloads) is the engine's; which payload owns which slot, whether a staged copy is still the
payload's, and whether a round may use it are decided here, without the device.
"""

from __future__ import annotations

import enum
from dataclasses import dataclass
from typing import Any, Callable

from .staging import baseline_key, payload_fingerprint


@dataclass(slots=True)
class Arrival:
    payload: Any      # kept alive: its id() is the key
    codec: Any
    signature: Any    # of the layout it was staged in
    rows: Any         # the engine's own: where the staged copy lives
    slot: Any         # goes back to the codec's free list (None: the engine holds no slot of its own)
    fingerprint: tuple
    delta_key: Any    # baseline_key of the model the row is a delta against; None: the row holds weights


class ArrivalTable(dict):
    """One engine's staged arrivals, ``id(payload) -> Arrival``, with its free slots per codec
    (:attr:`free`) and the key of the model staged as the arrival baseline (:attr:`base_key`)."""

    def __init__(self):
        super().__init__()
        self.reset()

    def reset(self) -> None:
        """Forget everything (the engine's layout changed: its slabs are gone)."""
        self.clear()
        self.free: dict[Any, list] = {}
        self.base_key = None

    def take(self, codec, grow: Callable[[], list]):
        """A free slot of ``codec``; ``grow()`` allocates one more slab and returns its slots."""
        free = self.free.setdefault(codec, [])
        if not free:
            free.extend(grow())
        return free.pop()

    def file(self, payload, codec, signature, rows, slot=None, delta_key=None) -> None:
        self[id(payload)] = Arrival(payload, codec, signature, rows, slot, payload_fingerprint(payload), delta_key)

    def lookup(self, payload, codec, signature) -> Arrival | None:
        """``payload``'s record if a round of this codec and layout would stage what was staged: the same
        object, and no entry replaced or written since (the fingerprint)."""
        rec = self.get(id(payload))
        if rec is None or rec.payload is not payload or rec.codec != codec or rec.signature != signature:
            return None
        return rec if rec.fingerprint == payload_fingerprint(payload) else None

    def drop(self, payload) -> None:
        """Return ``payload``'s slot; a record filed under its id for another object stays."""
        rec = self.get(id(payload))
        if rec is not None and rec.payload is payload:
            self._free(self.pop(id(payload)))

    def release(self) -> None:
        """Return every slot (after the round that used them has completed, or failed)."""
        for rec in self.values():
            self._free(rec)
        self.clear()

    def _free(self, rec: Arrival) -> None:
        if rec.slot is not None:
            self.free.setdefault(rec.codec, []).append(rec.slot)

    def free_count(self) -> int:
        return sum(len(slots) for slots in self.free.values())

    def baseline(self, model, layout, stage: Callable[[Any], None]):
        """The key of ``model`` as the arrival baseline, staged by ``stage(model)`` once per model version;
        None if it has no key (no version counters) or does not fit ``layout``: arrivals stay weights."""
        key = baseline_key(model)
        if key is None or key == self.base_key:
            return key
        try:
            layout.check_compatible(model, "baseline")
        except (KeyError, ValueError):
            return None
        stage(model)  # copy-stream order: rows converted against the previous model ran before this copy
        self.base_key = key
        return key


class Adopt(enum.Enum):
    AS_FORMED = 1  # a delta formed against this round's baseline
    CONVERT = 2    # weights: a delta round turns the row into its delta in place, a weight round uses it
    REFUSE = 3     # a delta against another model: the caller stages the payload again


def adopt_rule(delta_key, holds_deltas: bool, has_baseline: bool, base_key, same_bits: Callable[[], bool]) -> Adopt:
    """Whether a round (``holds_deltas``, ``has_baseline``, ``base_key``) may use an arrival row.

    ``same_bits()`` compares the staged arrival baseline with the round's on the device: matching keys
    (storage and version counters) do not exclude a write that left the counters alone or a freed storage
    reused at the same address.  It is called only when the keys match; the round caches its answer.
    """
    if delta_key is None:
        return Adopt.CONVERT
    if holds_deltas and has_baseline and delta_key == base_key and same_bits():
        return Adopt.AS_FORMED
    return Adopt.REFUSE


def stage_as_arrivals(engine, rnd, payloads) -> bool:
    """Stage a round's clients in slot order as arrival rows, so that the round that follows on ``engine``
    adopts them and nothing is staged twice (the detector server's attack simulation and filter, which run
    ahead of the aggregation): the row staged at arrival if the round may use it, else a fresh arrival row;
    a payload that does not fit the arrival slabs goes into the round's own slab.  Returns whether every
    payload lies in an arrival row."""
    in_arrival_rows = True
    for slot, payload in enumerate(payloads):
        if rnd.adopt(slot, payload):
            continue
        engine.drop_arrival(payload)  # staged as a delta, or written since: stage it again
        if engine.prestage(payload, rnd.layout) and rnd.adopt(slot, payload):
            continue
        rnd.put_client(slot, payload)
        in_arrival_rows = False
    return in_arrival_rows


def adopt_or_put(rnd, payloads, what: str | None = None) -> None:
    """Stage a round's clients in slot order: the copy staged at arrival if any, else the payload now."""
    extra = () if what is None else (what,)
    for slot, payload in enumerate(payloads):
        if not rnd.adopt(slot, payload):
            rnd.put_client(slot, payload, *extra)
