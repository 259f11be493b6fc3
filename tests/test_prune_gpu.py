"""plato_agg_prune_global on the GPU: every reference fixture bit for bit (the entries between the pieces
included), the drop-in processor over successive calls, and the kernel's seams against the numpy
restatement (tests/prune_oracle.py): sizes around the tile W and the grid G x W, unaligned and one-element
pieces, the extreme counts, keys that differ in one radix digit only, full and partial ties, a zero
threshold, and two identical runs."""

import numpy as np
import pytest
import torch

from plato_amd import prune as host
from plato_amd.processors.prune import Processor
from tests import prune_cases as pc
from tests import prune_oracle as po

pytestmark = pytest.mark.gpu

W, G = host.TILE, host.GRID
DEV = "cuda:0"


def device_prune(row_bits: np.ndarray, pieces, k: int):
    """The row pruned on the device: its bits and the record."""
    row = torch.from_numpy(row_bits.view(np.float32)).to(DEV)
    res = host.prune_row(row, pieces, k)
    return row.cpu().numpy().view(np.uint32), (res.threshold_key, res.below, res.ties, res.ties_pruned)


def check(row_bits, pieces, k):
    got, record = device_prune(row_bits, pieces, k)
    exp, exp_record = po.prune_row(row_bits, pieces, k)
    assert record == exp_record
    assert got.tobytes() == exp.tobytes()
    return got, record


def normal_bits(n, seed, scale=0.05):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32).view(np.uint32)


# ------------------------------------------------------------------ the reference fixtures
@pytest.mark.parametrize("name", pc.case_ids())
def test_fixture_rows_equal_the_reference(name):
    c = pc.case(name)
    names = c["prunable"]
    before = pc.state_bits(c, "in")
    for a in range(1, c["applications"] + 1):
        after = pc.state_bits(c, f"out{a}")
        row, pieces, where = pc.as_row(before, names)
        # NaN payloads between the pieces must survive: put some into the first entry that is not pruned
        spare = next(k for k in before if k not in names)
        row = row.copy()
        row[where[spare][0]] = 0x7FA00001
        got, record = device_prune(row, pieces, c["k"])
        for key, (b, e) in where.items():
            if key == spare:
                assert got[b:e].tobytes() == row[b:e].tobytes(), (name, a, key)
            else:
                assert got[b:e].tobytes() == after[key].view(np.uint32).tobytes(), (name, a, key)
        if c["k"]:
            assert dict(zip(("T", "below", "ties", "r"), record)) == c["records"][a - 1]
        before = after


@pytest.mark.parametrize("name", ["toy_thrice", "toy_nonfinite_twice", "resblock_half", "toy_half_up", "lenet5_most"])
def test_drop_in_reproduces_tensors_and_key_order(name):
    c = pc.case(name)

    class Trainer:
        model = pc.load_model(c)

    proc = Processor(amount=pc.amount_of(c), name="unstructured_pruning", trainer=Trainer(), server_id=0)
    for a in range(1, c["applications"] + 1):
        out = proc.process(None)
        exp = pc.state_bits(c, f"out{a}")
        assert list(out) == c["keys_out"][a - 1] == list(Trainer.model.state_dict())
        got = pc.model_bits(Trainer.model)
        for key in exp:
            assert got[key].tobytes() == exp[key].tobytes(), (name, a, key)
            assert not out[key].is_cuda
        assert proc.last_result.k == c["k"] and proc.last_result.threshold_key == c["records"][a - 1]["T"]


def test_drop_in_over_three_calls_on_a_device_model():
    """The toy model living on the GPU: three successive calls, tensors and key order of each."""
    c = pc.case("toy_thrice")

    class Trainer:
        model = pc.load_model(c).to(DEV)

    proc = Processor(amount=pc.amount_of(c), trainer=Trainer(), server_id=0)
    for a in range(1, 4):
        out = proc.process(None)
        exp = pc.state_bits(c, f"out{a}")
        assert list(out) == c["keys_out"][a - 1]
        got = pc.model_bits(Trainer.model)
        assert all(got[key].tobytes() == exp[key].tobytes() for key in exp)
        Trainer.model.to(DEV)  # process() leaves it on the CPU, as the reference does


# ------------------------------------------------------------------ seams against the oracle
@pytest.mark.parametrize("n", [1, 3, W - 1, W, W + 1, 2 * G * W + 5])
def test_sizes_around_the_tile_and_the_grid(n):
    bits = normal_bits(n + 8, 100 + n % 97)
    if n <= W + 1:
        for k in sorted({1, n // 3 + 1, n}):
            check(bits, [(4, 4 + n)], k)
        return
    # more tiles than workgroups: a partial tie planted in tiles of every grid step, half of it pruned
    planted = np.arange(4 + 13, 4 + n, 97 * W + 13)
    bits[planted] = 0x3CA3D70A
    ky = po.keys(bits[4:4 + n])
    k = int(np.count_nonzero(ky < 0x3CA3D70A)) + int(np.count_nonzero(ky == 0x3CA3D70A)) // 2
    got, record = check(bits, [(4, 4 + n)], k)
    assert record[0] == 0x3CA3D70A and 0 < record[3] < record[2]


@pytest.mark.parametrize("n", [1, 3, W + 1])
@pytest.mark.parametrize("k_of", ["0", "1", "n-1", "n"])
def test_counts(n, k_of):
    k = {"0": 0, "1": 1, "n-1": n - 1, "n": n}[k_of]
    bits = normal_bits(n + 3, 7 + n)
    got, record = check(bits, [(3, 3 + n)], k)
    assert int(np.count_nonzero(po.keys(got[3:]) == 0)) >= k


def test_unaligned_pieces_and_a_one_element_piece():
    """Begin offsets 1, 2 and 3 elements past a 16-byte boundary, pieces longer than a tile and shorter than
    a vector, a one-element piece, an empty one, and gaps whose bits must survive."""
    n_row = 3 * W + 64
    bits = normal_bits(n_row, 31)
    bits[::7] |= 0x7FA00000  # NaNs with payloads everywhere, in the gaps too
    pieces = [(1, 6), (10, 11), (14, 14), (18, 18 + W + 3), (W + 31, W + 33), (W + 35, 3 * W + 63)]
    assert [b % 4 for b, _ in pieces] == [1, 2, 2, 2, 3, 3]
    n = sum(e - b for b, e in pieces)
    for k in (1, n // 2, n - 1, n):
        got, _ = check(bits, pieces, k)
        gaps = np.ones(n_row, dtype=bool)
        for b, e in pieces:
            gaps[b:e] = False
        assert got[gaps].tobytes() == bits[gaps].tobytes()


@pytest.mark.parametrize("which", ["lowest", "highest", "middle"])
def test_keys_that_differ_in_one_radix_digit(which):
    """The digits are 11, 10 and 10 bits wide: keys equal but for one of them."""
    n = 2 * W + 77
    rng = np.random.default_rng(5)
    shift, width = {"lowest": (0, 10), "middle": (10, 10), "highest": (20, 11)}[which]
    fixed = 0x3D2AA955 & ~(((1 << width) - 1) << shift)
    bits = (fixed | (rng.integers(0, 1 << width, n).astype(np.uint32) << shift)).astype(np.uint32)
    bits |= rng.integers(0, 2, n).astype(np.uint32) << 31  # signs do not rank
    for k in (1, n // 5, n - 1):
        check(bits, [(0, n)], k)


def test_full_tie():
    n = W + 9
    bits = np.full(n, 0x3E99999A, dtype=np.uint32)
    bits[1::2] |= 0x80000000
    for k in (1, 2, n // 2, n):
        got, record = check(bits, [(0, n)], k)
        assert record == (0x3E99999A, 0, n, k)
        assert np.all(po.keys(got[:k]) == 0) and got[k:].tobytes() == bits[k:].tobytes()  # the lowest indices


def test_partial_tie_across_workgroups_and_pieces():
    """0 < r < ties with the tied elements in different tiles (so different workgroups) and pieces.  Against
    the oracle's lowest-index rule, and for what also holds for the reference: exactly k pruned, all below T
    and none above."""
    n_row = 6 * W
    bits = normal_bits(n_row, 77, scale=1.0)
    bits[po.keys(bits) == 0x3F000000] += 1
    pieces = [(2, W + 7), (W + 9, 3 * W + 1), (3 * W + 2, 6 * W - 3)]
    tied = [3, 4, 5, 200, W - 1, W + 6, W + 9, 2 * W + 17, 3 * W, 3 * W + 2, 4 * W + 5, 4 * W + 6, 5 * W + 1, 6 * W - 4]
    bits[tied] = 0x3F000000
    bits[tied[::2]] |= 0x80000000
    idx = np.concatenate([np.arange(b, e) for b, e in pieces])
    assert set(tied) <= set(idx.tolist())
    below = int(np.count_nonzero(po.keys(bits[idx]) < 0x3F000000))
    for r in (1, 2, 5, 6, 7, 13):
        k = below + r
        got, record = check(bits, pieces, k)
        assert record == (0x3F000000, below, len(tied), r)
        pruned = got[idx] != bits[idx]
        ky = po.keys(bits[idx])
        assert int(pruned.sum()) == k
        assert np.all(pruned[ky < 0x3F000000]) and not np.any(pruned[ky > 0x3F000000])
        assert np.flatnonzero(got[tied] != bits[tied]).tolist() == list(range(r))  # the lowest flat indices


def test_zero_threshold_with_more_zeros_than_k():
    n = 2 * W + 3
    bits = normal_bits(n, 41)
    zeros = np.random.default_rng(3).choice(n, 900, replace=False)
    bits[zeros] = 0
    bits[zeros[::2]] = 0x80000000
    for k in (1, 450, 899, 900, 901):
        got, record = check(bits, [(0, n)], k)
        assert record[0] == 0 or k == 901
        if k <= 900:
            assert got.tobytes() == bits.tobytes()  # +-0 * 0 keeps its bits


def test_two_runs_are_identical():
    n = 3 * W + 11
    bits = normal_bits(n, 9)
    bits[:: 5] = 0x3DCCCCCD  # many ties at one value
    k = int(np.count_nonzero(po.keys(bits[1:n - 2]) < 0x3DCCCCCD)) + 100
    first = device_prune(bits, [(1, n - 2)], k)
    second = device_prune(bits, [(1, n - 2)], k)
    assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]
    assert first[1][3] == 100 and first[1][2] > 100


def test_resnet18_size_against_kthvalue():
    """ResNet-18's prunable size with random weights: T and #(key < T) against torch.kthvalue on the host,
    the row against the oracle."""
    from plato_amd import workloads

    shapes = [s for name, s, kind in workloads.resnet(18, 10)
              if kind == "f32" and name.endswith("weight") and len(s) in (2, 4)]
    sizes = [int(np.prod(s)) for s in shapes]
    n = sum(sizes)
    assert len(sizes) == 21 and n == 11_164_352
    bits = normal_bits(n + 21 * 3, 2024, scale=0.02)
    pieces, at = [], 0
    for s in sizes:  # three untouched elements before every piece: the pieces start at every alignment
        pieces.append((at + 3, at + 3 + s))
        at += 3 + s
    k = host.nparams_toprune(0.2, n)
    got, record = device_prune(bits, pieces, k)
    idx = np.concatenate([np.arange(b, e) for b, e in pieces])
    ky = torch.from_numpy(po.keys(bits[idx]).astype(np.int64))
    t = int(torch.kthvalue(ky, k).values)
    assert record[0] == t and record[1] == int((ky < t).sum()) and record[2] == int((ky == t).sum())
    exp, exp_record = po.prune_row(bits, pieces, k)
    assert record == exp_record and got.tobytes() == exp.tobytes()
