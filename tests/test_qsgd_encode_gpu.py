"""plato_agg_qsgd_encode on the GPU: every reference fixture byte for byte through ``encode_state_dict`` and
through the drop-in processor, and the kernel's seams against the numpy restatement
(tests/qsgd_encode_oracle.py), codes and maxima both: sizes around the tile W and the grid G x W, every begin
offset, adjacent pieces that share a dword of the codes, empty pieces, gaps that keep their bytes, the
maximum in every kind of tile, all-zero and non-finite pieces, levels 2 and 128, determinism, and the chain
into the project's own QSGD decoder and FedAvg round."""

import numpy as np
import pytest
import torch

from oracle import fedavg_oracle as ref
from oracle import qsgd as Q
from plato_amd import qsgd_encode as host
from plato_amd import weights as Wt
from plato_amd.arena import ArenaLayout
from plato_amd.engine import FedAvgEngine
from plato_amd.processors.qsgd import Processor as Dequantize
from plato_amd.processors.qsgd_encode import Processor
from tests import golden_cases as G
from tests import qsgd_encode_cases as qc
from tests import qsgd_encode_oracle as qo

pytestmark = pytest.mark.gpu

W, G_ = host.TILE, host.GRID
DEV = "cuda:0"
FILL = 0xA5


def normal_bits(n, seed, scale=0.05):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32).view(np.uint32)


def device_encode(row_bits, pieces, level, seed):
    """Codes (over a row of codes pre-filled with 0xA5) and maxima from the device."""
    row = torch.from_numpy(row_bits.view(np.float32).copy()).to(DEV)
    codes = torch.full((row_bits.size,), FILL, dtype=torch.uint8, device=DEV)
    got, keys = host.encode_row(row, pieces, level, seed, codes)
    assert got.data_ptr() == codes.data_ptr()
    return got.cpu().numpy(), keys.cpu().numpy().view(np.uint32)


def check(row_bits, pieces, level, seed, unspecified=()):
    """Device against oracle, byte for byte: the maxima, the codes of every piece not in ``unspecified`` and
    the 0xA5 of every byte outside the pieces."""
    got, keys = device_encode(row_bits, pieces, level, seed)
    exp, exp_keys = qo.encode_row(row_bits, pieces, level, seed, np.full(row_bits.size, FILL, dtype=np.uint8))
    assert keys.tolist() == exp_keys.tolist()
    for p in unspecified:
        b, e = pieces[p]
        got[b:e] = exp[b:e]
    assert got.tobytes() == exp.tobytes()
    return got, keys


# ------------------------------------------------------------------ the reference fixtures
@pytest.mark.parametrize("name", qc.case_ids())
def test_fixtures_through_encode_state_dict(name):
    c = qc.case(name)
    exp = qc.wire(c)
    got = host.encode_state_dict(qc.state_dict(c), c["level"], c["draw_seed"], DEV)
    assert list(got) == list(exp)
    for key in exp:
        assert isinstance(got[key], bytes) and got[key] == exp[key], (name, key)


@pytest.mark.parametrize("name", qc.case_ids())
def test_fixtures_through_the_drop_in(name, monkeypatch):
    """The processor's seed schedule is splitmix64(seed + call): the fixture's draw seed is planted as the
    seed of the second call, and the first call (another seed) gives other bytes."""
    c = qc.case(name)
    exp = qc.wire(c)
    proc = Processor(quantization_level=c["level"], server_id=0, seed=99, device=DEV)
    first = proc.process(qc.state_dict(c))
    assert list(first) == list(exp) and proc.calls == 1
    assert proc.last_seed == Processor(seed=99).next_seed() != c["draw_seed"]
    monkeypatch.setattr(proc, "next_seed", lambda: c["draw_seed"])
    got = proc.process(qc.state_dict(c))
    assert proc.last_seed == c["draw_seed"]
    for (key, _, shape) in c["entries"]:
        assert got[key] == exp[key], (name, key)
        head = 10 + 2 * len(shape)
        assert first[key][:head] == exp[key][:head] and len(first[key]) == len(exp[key])  # the seed moves no header
    assert any(first[key] != exp[key] for key in exp)


def test_drop_in_on_device_tensors_and_fresh_seeds():
    """A state that lives on the GPU gives the same bytes; without a seed two calls differ and keep theirs."""
    c = qc.case("toy_l64")
    on_device = {k: t.to(DEV) for k, t in qc.state_dict(c).items()}
    got = host.encode_state_dict(on_device, c["level"], c["draw_seed"], DEV)
    assert list(got.items()) == list(qc.wire(c).items())
    proc = Processor(client_id=4, device=DEV)
    a = proc.process(qc.state_dict(c))
    seed_a = proc.last_seed
    b = proc.process(qc.state_dict(c))
    assert seed_a != proc.last_seed and a != b
    assert a == host.encode_state_dict(qc.state_dict(c), 64, seed_a, DEV)


# ------------------------------------------------------------------ seams against the oracle
@pytest.mark.parametrize("n", [1, 3, 4, 5, W - 1, W, W + 1, 2 * W + 3])
def test_sizes_around_the_tile_at_every_begin_offset(n):
    for offset, level in zip(range(4), (64, 2, 128, 37)):
        bits = normal_bits(offset + n + 9, 100 + n % 97 + offset)
        check(bits, [(4 + offset, 4 + offset + n)], level, seed=n + offset)


def test_one_piece_that_needs_a_second_grid_step():
    n = G_ * W + W + 1
    bits = normal_bits(n + 6, 21)
    bits[3 + n - 1] = 0xBF800000  # the maximum is the last element, in the guarded tile of the second step
    got, keys = check(bits, [(3, 3 + n)], 64, seed=5)
    assert keys.tolist() == [0x3F800000] and got[3 + n - 1] == 0x80 | 63


@pytest.mark.parametrize("where", ["first tile", "last guarded tile", "a full tile of another workgroup"])
def test_the_maximum_in_every_kind_of_tile(where):
    n = 3 * W + 3
    bits = normal_bits(n + 8, 33, scale=0.01)
    at = {"first tile": 2, "last guarded tile": 2 + n - 2, "a full tile of another workgroup": 2 + W + W // 2}[where]
    bits[at] = 0x40490FDB
    got, keys = check(bits, [(2, 2 + n)], 128, seed=8)
    assert keys.tolist() == [0x40490FDB] and got[at] == 127


def test_adjacent_small_pieces_share_code_dwords():
    """Runs of adjacent pieces of 1 to 3 elements with maxima that differ by orders of magnitude, empty pieces
    among them, one-byte gaps, then pieces that meet in the middle of a dword after a full tile."""
    rng = np.random.default_rng(6)
    pieces, at = [], 1
    for i in range(120):
        n = int(rng.integers(1, 4))
        pieces.append((at, at + n))
        at += n
        if i % 7 == 3:
            pieces.append((at, at))  # empty
        if i % 11 == 5:
            at += 1  # a gap of one byte that must keep 0xA5
    pieces.append((at + 1, at + 1 + W + 6))  # full tiles inside, ends in the middle of a dword
    at = pieces[-1][1]
    pieces.append((at, at + 2))
    pieces.append((at + 2, at + 2))
    pieces.append((at + 2, at + 5))
    n_row = at + 9
    bits = normal_bits(n_row, 12, scale=1.0)
    vals = bits.view(np.float32)
    for p, (b, e) in enumerate(pieces):
        vals[b:e] *= np.float32(10.0) ** (p % 9 - 4)
    for level in (2, 64, 128):
        got, keys = check(bits, pieces, level, seed=level)
        assert len(set(keys.tolist())) > 100
    assert all(keys[p] == 0 for p, (b, e) in enumerate(pieces) if e == b)


@pytest.mark.parametrize("level", [2, 128])
def test_all_zero_and_non_finite_pieces(level):
    """An all-zero piece (both signs of zero) gets zero codes and key 0.  A piece with a NaN or an infinity
    reports a key >= 0x7f800000 and writes only inside itself; the pieces around it are exact."""
    n_row = 2 * W + 40
    bits = normal_bits(n_row, 51)
    pieces = [(1, 7), (7, 18), (18, 21), (21, 21 + W + 5), (W + 26, W + 30), (W + 30, 2 * W + 37)]
    bits[7:18] = 0
    bits[8:18:2] = 0x80000000
    bits[19] = 0x7FC00001                     # a NaN in a three-element piece
    bits[W + 27] = 0xFF800000                 # -inf in a four-element piece
    got, keys = check(bits, pieces, level, seed=3, unspecified=(2, 4))
    assert keys[1] == 0 and not got[7:18].any()
    assert keys[2] == 0x7FC00001 and keys[4] == 0x7F800000
    assert all(0 < k < 0x7F800000 for k in keys[[0, 3, 5]])
    if level == 128:
        big = bits.copy()
        big[21 + 5] = 0xC0000000  # -2.0 is the maximum of piece 3: the byte 0xFF
        got, _ = check(big, pieces, level, seed=3, unspecified=(2, 4))
        assert got[21 + 5] == 0xFF


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")], ids=["nan", "inf", "-inf"])
def test_non_finite_entry_raises_and_names_the_entry(value):
    c = qc.case("toy_l64")
    sd = qc.state_dict(c)
    name = list(sd)[2]
    sd[name].view(-1)[1] = value
    with pytest.raises(ValueError, match=f"{name!r} holds an infinity or a NaN"):
        host.encode_state_dict(sd, 64, 1, DEV)
    proc = Processor(seed=1, device=DEV)
    with pytest.raises(ValueError, match=f"{name!r}"):
        proc.process(sd)
    assert proc.last_seed is None and proc.calls == 1  # the refused call used up its seed and kept none


def test_all_zero_entry_is_encoded_and_decodes_to_zeros():
    sd = {"w": torch.tensor([0.5, -0.25, 0.0]), "bias": torch.zeros(2, 3), "n": torch.tensor(0), "e": torch.zeros(0)}
    got = host.encode_state_dict(sd, 64, 2, DEV)
    assert got["bias"] == host.header(0, (2, 3)) + bytes(6) and got["n"] == host.header(0, ()) + bytes(1)
    assert got["e"] == host.header(0, (0,))
    assert not Q.decode_layer(got["bias"]).any() and Q.decode_layer(got["bias"]).shape == (2, 3)
    assert got["w"] == qo.encode_state({k: t.numpy() for k, t in sd.items()}, 64, 2)["w"]
    empty_only = host.encode_state_dict({"e": torch.zeros(0), "f": torch.zeros(3, 0)}, 64, 2, DEV)
    assert empty_only == {"e": host.header(0, (0,)), "f": host.header(0, (3, 0))}


# ------------------------------------------------------------------ determinism
def test_determinism_and_independence_of_the_other_pieces():
    n_row = 2 * W + 50
    bits = normal_bits(n_row, 71)
    pieces = [(0, 5), (5, 9), (11, 11 + W + 1), (W + 13, 2 * W + 47)]
    first = device_encode(bits, pieces, 64, 10)
    second = device_encode(bits, pieces, 64, 10)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tolist() == second[1].tolist()
    other = device_encode(bits, pieces, 64, 11)
    assert other[1].tolist() == first[1].tolist()  # the maxima do not depend on the seed
    differ = np.count_nonzero(other[0] != first[0])
    assert n_row // 8 < differ  # about half of the elements round the other way
    # a piece encoded alone at the same row position gives the same bytes as among the others
    for p, (b, e) in enumerate(pieces):
        alone, key = device_encode(bits, [(b, e)], 64, 10)
        assert alone[b:e].tobytes() == first[0][b:e].tobytes() and key.tolist() == [first[1][p]]
        assert np.all(alone[:b] == FILL) and np.all(alone[e:] == FILL)


def test_fresh_codes_are_zero_outside_the_pieces():
    bits = normal_bits(64, 2)
    row = torch.from_numpy(bits.view(np.float32).copy()).to(DEV)
    codes, keys = host.encode_row(row, [(3, 30), (40, 40)], 64, 4)
    exp, exp_keys = qo.encode_row(bits, [(3, 30), (40, 40)], 64, 4, np.zeros(64, dtype=np.uint8))
    assert codes.cpu().numpy().tobytes() == exp.tobytes() and keys.cpu().numpy().view(np.uint32).tolist() == exp_keys.tolist()
    codes, keys = host.encode_row(row, [], 64, 4)
    assert not codes.any() and keys.numel() == 0
    codes, keys = host.encode_row(row, [(5, 5), (9, 9)], 64, 4)
    assert not codes.any() and keys.tolist() == [0, 0]


# ------------------------------------------------------------------ the chain into the decoder
def _flat(layout, sd, region):
    parts = [sd[e.name].reshape(-1).float() for e in layout.entries if e.region == region]
    return torch.cat(parts).numpy() if parts else np.zeros(0, np.float32)


def test_chain_encode_decode_fedavg():
    """Two toy models quantized on the device, their wire dicts through the project's QSGD inbound processor
    and the QSGD FedAvg round: bit for bit the oracle's encode, the reference's decode (oracle/qsgd.py) and
    the FedAvg oracle."""
    level, k = 64, 2
    states = [qc.seeded_state({"state": "toy", "seed": 7001 + i}) for i in range(k)]
    spec = [(name, tuple(a.shape), "f32" if a.dtype == np.float32 else "i64") for name, a in states[0].items()]
    layout = ArenaLayout.from_shapes(spec)
    rng = np.random.default_rng(7)
    bf = (rng.standard_normal(layout.n_f32) * 0.1).astype(np.float32)
    bi = rng.integers(0, 500, layout.n_i64)
    baseline = layout.unpack(torch.from_numpy(bf), torch.from_numpy(bi))
    wires = [host.encode_state_dict({n: torch.from_numpy(np.array(a)) for n, a in st.items()}, level, 40 + i, DEV)
             for i, st in enumerate(states)]
    for i, st in enumerate(states):
        assert list(wires[i].items()) == list(qo.encode_state(st, level, 40 + i).items())
    deq = []
    for w in wires:
        vals = {n: Q.decode_layer(b, level).reshape(-1) for n, b in w.items()}
        deq.append((np.concatenate([vals[e.name] for e in layout.entries if e.region == "f32"]),
                    np.concatenate([vals[e.name] for e in layout.entries if e.region == "i64"])))
    proc = Dequantize(quantization_level=level)
    engine = FedAvgEngine(DEV)
    rnd = engine.begin(baseline, k, "qsgd")
    rnd.put_baseline(baseline)
    for slot in range(k):
        rnd.put_client(slot, proc.process(wires[slot]))
    weights = Wt.fedavg([300, 700])
    rnd.launch(weights)
    got = rnd.result()
    exp_f, exp_i = ref.fedavg_numpy(bf, bi, [d[0] for d in deq], [d[1] for d in deq], weights)
    assert G.canon(_flat(layout, got, "f32")).tobytes() == G.canon(exp_f).tobytes()
    assert G.canon(_flat(layout, got, "i64")).tobytes() == G.canon(exp_i).tobytes()
