"""Server-side behaviour of the hooks on the GPU: the event loop keeps running, arrivals are
released on error, and a payload edited after its arrival copy is staged again.

* Plato's server is one asyncio loop (plato/servers/base.py:323-327) that also serves the
  clients' sockets; the reference's aggregation yields to it per client
  (plato/servers/fedavg.py:157).  The hooks here run every pack, H2D, device reduction
  and host sync on the aggregation worker thread; a ticker coroutine must keep ticking
  through a FedAtt and a Port round (their device reductions end in host syncs).
* A round whose weights raise (FedAdp without ``lr``, a bad stored model) must not leak
  the HBM arrival slots or the payload references they hold.
* ``prestage`` copies a payload when it arrives; a processor or hook may replace an
  entry or write one in place afterwards — the round must aggregate the current values.
"""

import asyncio
import time
import types

import numpy as np
import pytest
import torch

from oracle import fedavg_oracle as ref
from oracle import synth
from plato_amd.arena import ArenaLayout
from plato_amd.engine import FedAvgEngine
from tests import golden_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {c["recipe"]["name"]: c for c in G.load_cases()}


def _flat(layout, sd, region):
    parts = [sd[e.name].reshape(-1).float() for e in layout.entries if e.region == region]
    return torch.cat(parts).numpy() if parts else np.zeros(0, np.float32)


async def _with_ticker(coro, period=0.001):
    """Run ``coro`` while a ticker coroutine records when the loop let it run."""
    ticks = []
    done = False

    async def ticker():
        while not done:
            ticks.append(time.perf_counter())
            await asyncio.sleep(period)

    task = asyncio.ensure_future(ticker())
    await asyncio.sleep(0)
    t0 = time.perf_counter()
    try:
        result = await coro
    finally:
        done = True
        await task
    t1 = time.perf_counter()
    inside = [t for t in ticks if t0 <= t <= t1]
    edges = [t0] + inside + [t1]
    max_gap = max(b - a for a, b in zip(edges, edges[1:]))
    return result, len(inside), max_gap, t1 - t0


def test_fedatt_round_leaves_the_event_loop_running():
    from plato_amd.algorithms.fedavg import FedAttAlgorithmMixin

    name = "fedatt_resnet18_k8"
    recipe, exp = CASES[name]["recipe"], CASES[name]["expected"]
    layout, base, pays, _ = G.host_state_dicts(recipe)

    class Algorithm(FedAttAlgorithmMixin):
        aggregation_device = DEV

    alg = Algorithm()
    torch.manual_seed(recipe["noise_seed"])
    asyncio.run(alg.aggregate_weights(base, pays))  # warm: engine, arenas, pinned ring
    torch.manual_seed(recipe["noise_seed"])
    updated, n_ticks, max_gap, total = asyncio.run(_with_ticker(alg.aggregate_weights(base, pays)))
    assert G.sha(G.canon(_flat(layout, updated, "f32"))) == exp["updated_f32_sha256"]
    assert n_ticks >= 3, (n_ticks, total)
    assert max_gap < 0.1, (max_gap, total)
    assert alg.aggregation_engine()._arrivals == {}


def test_port_round_leaves_the_event_loop_running(tmp_path):
    from plato_amd.servers.variants import PortServerMixin

    case = CASES["port_similarity_resnet18_k4"]
    recipe = case["recipe"]
    layout = ArenaLayout.from_shapes(G.model_spec(recipe["model"]))
    _, base, pays, _ = G.host_state_dicts(recipe)
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, recipe["seed"])
    pv = recipe["previous"]
    prev = layout.unpack(torch.from_numpy(synth.synth_f32(layout.n_f32, recipe["seed"], pv["stream"], pv["scale"],
                                                          add=bf)),
                         torch.from_numpy(synth.synth_i64(layout.n_i64, recipe["seed"], pv["stream"], 3, add=bi)))
    path = tmp_path / "model_prev.pth"
    torch.save(prev, path)
    st = recipe["staleness"]
    updates = [types.SimpleNamespace(client_id=c + 1, staleness=st[c],
                                     report=types.SimpleNamespace(num_samples=recipe["num_samples"][c]))
               for c in G.order_of(recipe)]

    class Server(PortServerMixin):
        aggregation_device = DEV
        staleness_weight = 3
        current_round = recipe["current_round"]
        port_threads = 8

        def port_previous_model_path(self):
            return str(path)

    server = Server()
    asyncio.run(server.aggregate_weights(updates, base, pays))
    updated, n_ticks, max_gap, total = asyncio.run(_with_ticker(server.aggregate_weights(updates, base, pays)))
    assert G.sha(G.canon(_flat(layout, updated, "f32"))) == case["expected"]["updated_f32_sha256"]
    assert n_ticks >= 3, (n_ticks, total)
    assert max_gap < 0.1, (max_gap, total)


def test_raising_weights_release_the_arrival_slots():
    from plato_amd.servers.fedavg import FusedAggregationMixin

    recipe = CASES["resnet18_k16_permuted"]["recipe"]
    layout, base, pays, _ = G.host_state_dicts(recipe)
    blay = ArenaLayout.from_state_dict(base)

    class Boom(RuntimeError):
        pass

    class Server(FusedAggregationMixin):
        aggregation_device = DEV

        def aggregation_weights(self, updates):
            raise Boom("weights failed")

    server = Server()
    eng = server.aggregation_engine()
    for p in pays:
        assert eng.prestage(p, blay)
    assert len(eng._arrivals) == len(pays)
    updates = [types.SimpleNamespace(client_id=c + 1, report=types.SimpleNamespace(num_samples=1))
               for c in range(len(pays))]
    with pytest.raises(Boom):
        asyncio.run(server.aggregate_weights(updates, base, pays))
    assert eng._arrivals == {}
    # the freed slots serve the next round, which sees only its own payloads
    assert eng._arrivals.free_count() >= len(pays)


def _arrival_slab_counts(eng, engine_kind) -> list:
    """Arrival slabs allocated so far, per place that allocates them (engine, bucket shard, entry shard)."""
    if engine_kind == "single":
        return [sum(len(v) for v in eng._arrival_slabs.values())]
    if engine_kind == "multi":
        return [sum(len(v) for v in s.arrival_slabs.values()) for s in eng._shards]
    return [sum(len(v) for v in e._arrival_slabs.values()) for e in eng._engines]


@pytest.mark.parametrize("deltas", [False, True], ids=["weights", "deltas"])
@pytest.mark.parametrize("engine_kind", ["single", "multi", "entry"])
def test_seventeen_arrivals_fill_a_second_slab_and_are_all_adopted(engine_kind, deltas):
    """One arrival more than a slab holds (ARRIVAL_CHUNK = 16): the second slab is allocated, a round
    adopts rows of both slabs, and the released slots serve the next 17 arrivals without a third slab."""
    layout = ArenaLayout.from_shapes([("a", (37, 7), "f32"), ("n", (), "i64"), ("b", (3, 5), "f32")])
    k, seed = 17, 5
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, seed)
    xs = [synth.client_arena(bf, bi, seed, c) for c in range(k)]
    base = layout.unpack(torch.from_numpy(bf), torch.from_numpy(bi))
    pays = [layout.unpack(torch.from_numpy(xf), torch.from_numpy(xi)) for xf, xi in xs]
    if engine_kind == "single":
        eng = FedAvgEngine(DEV)
        eng.delta_arenas = deltas
    else:
        from plato_amd.multi import MultiDeviceEngine

        eng = MultiDeviceEngine([DEV, DEV])
        eng.delta_arenas = deltas
        if engine_kind == "entry":
            eng = eng.entries
    assert FedAvgEngine.ARRIVAL_CHUNK == 16 and k == FedAvgEngine.ARRIVAL_CHUNK + 1
    blay = ArenaLayout.from_state_dict(base)
    for p in reversed(pays):
        assert eng.prestage(p, blay, base if deltas else None)
    assert len(eng._arrivals) == k
    counts = _arrival_slab_counts(eng, engine_kind)
    assert set(counts) - {0} == {2}, counts
    rnd = eng.begin(base, k)
    rnd.put_baseline(base)
    assert [rnd.adopt(slot, p) for slot, p in enumerate(pays)] == [True] * k
    w = ref.fedavg_weights(synth.num_samples(k, seed))
    rnd.launch(w)
    got = rnd.result()
    eng.release_arrivals()
    assert len(eng._arrivals) == 0
    exp_f, exp_i = ref.fedavg_numpy(bf, bi, [x[0] for x in xs], [x[1] for x in xs], w)
    assert _flat(layout, got, "f32").tobytes() == exp_f.tobytes()
    assert _flat(layout, got, "i64").tobytes() == exp_i.tobytes()
    for p in reversed(pays):
        assert eng.prestage(p, blay, base if deltas else None)
    assert _arrival_slab_counts(eng, engine_kind) == counts
    eng.release_arrivals()


@pytest.mark.parametrize("edit", ["replace", "in_place"])
@pytest.mark.parametrize("engine_kind", ["single", "multi"])
def test_payload_edited_after_arrival_is_restaged(edit, engine_kind):
    recipe = CASES["resnet18_k16_permuted"]["recipe"]
    layout, base, pays, (bf, bi, xs_f, xs_i) = G.host_state_dicts(recipe)
    k = len(pays)
    if engine_kind == "single":
        eng = FedAvgEngine(DEV)
    else:
        from plato_amd.multi import MultiDeviceEngine

        eng = MultiDeviceEngine([DEV, DEV, DEV])
    blay = ArenaLayout.from_state_dict(base)
    for p in pays:
        assert eng.prestage(p, blay)
    # a hook changes client 3's first fp32 entry after its arrival copy
    e = next(e for e in layout.entries if e.region == "f32")
    if edit == "replace":
        pays[3][e.name] = pays[3][e.name] + 1.0
    else:
        pays[3][e.name].add_(1.0)
    xs_f = [x.copy() for x in xs_f]
    xs_f[3][e.offset:e.offset + e.numel] = pays[3][e.name].reshape(-1).numpy()
    rnd = eng.begin(base, k)
    rnd.put_baseline(base)
    adopted = []
    for slot, p in enumerate(pays):
        ok = rnd.adopt(slot, p)
        adopted.append(ok)
        if not ok:
            rnd.put_client(slot, p)
    assert adopted == [i != 3 for i in range(k)]
    w = [n / sum(recipe["num_samples"]) for n in recipe["num_samples"]]
    rnd.launch(w)
    got = rnd.result()
    eng.release_arrivals()
    exp_f, exp_i = ref.fedavg_numpy(bf, bi, xs_f, xs_i, w)
    assert _flat(layout, got, "f32").tobytes() == exp_f.tobytes()
    assert _flat(layout, got, "i64").tobytes() == exp_i.tobytes()
