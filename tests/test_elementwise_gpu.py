"""The elementwise entry points at their edges, through the C ABI: ``plato_agg_mix_weights`` (FedAsync,
examples/async/fedasync/fedasync_algorithm.py:9-20) with both outputs and scalar tails,
``plato_agg_cast_f32_i64`` (load_state_dict's truncating copy) around +-2^63 and over every power of
two, and ``plato_agg_fill_synth_{f32,i64}_at`` as slices of the streams written from element 0.
"""

import numpy as np
import pytest
import torch

from oracle import fedavg_oracle as ref
from oracle import synth
from plato_amd import _lib
from plato_amd.engine import cast_to_int64
from tests import edge_cases as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


@pytest.mark.parametrize("m", [0.54, 0.0, 1.0])
@pytest.mark.parametrize("n_i", [0, 1, 7])
@pytest.mark.parametrize("n_f", [1, 3, 5, 1027])
def test_mix_weights_both_outputs(n_f, n_i, m):
    rng = np.random.default_rng(1000 * n_f + 10 * n_i + int(100 * m))
    bf = rng.standard_normal(n_f).astype(np.float32)
    xf = rng.standard_normal(n_f).astype(np.float32)
    if n_f >= 5:  # 0 * inf, inf - inf, subnormals, signed zeros
        at = rng.choice(n_f, 4, replace=False)
        bf[at[:2]] = rng.choice(E.SPECIAL_F32, 2)
        xf[at[2:]] = rng.choice(E.SPECIAL_F32, 2)
    bi = rng.integers(-(1 << 40), 1 << 40, n_i, dtype=np.int64)
    xi = rng.integers(-(1 << 40), 1 << 40, n_i, dtype=np.int64)
    if n_i:  # above 2^24: the int64 -> fp32 cast rounds (ties to even) before the multiply
        bi[0], xi[0] = (1 << 24) + 1, -((1 << 24) + 3)
    if n_i > 2:
        bi[1], xi[1], bi[2], xi[2] = E.I64_MAX, E.I64_MIN, (1 << 53) + 1, 3
    dbf, dxf, dbi, dxi = (E.device_array(a, DEV) for a in (bf, xf, bi, xi))
    out_f, out_i = E.guarded(n_f, E.SENTINEL32, DEV), E.guarded(n_i, E.SENTINEL32, DEV)
    _lib.call("plato_agg_mix_weights", dxf.data_ptr(), dxi.data_ptr() if n_i else None, dbf.data_ptr(),
              dbi.data_ptr() if n_i else None, float(np.float32(1 - m)), float(np.float32(m)), out_f.data_ptr(),
              out_i.data_ptr() if n_i else None, n_f, n_i, _stream())
    torch.cuda.synchronize()
    got_f, got_i = E.fetch(out_f, np.uint32), E.fetch(out_i, np.uint32)
    assert (got_f[n_f:] == E.SENTINEL32).all() and (got_i[n_i:] == E.SENTINEL32).all(), "guard words overwritten"
    with np.errstate(all="ignore"):
        want_f, want_i = ref.mix_numpy(bf, bi, xf, xi, m)
    assert np.array_equal(E.bits32(got_f[:n_f].view(np.float32)), E.bits32(want_f))
    assert np.array_equal(E.bits32(got_i[:n_i].view(np.float32)), E.bits32(want_i))


def test_cast_to_int64_boundaries_and_powers_of_two():
    vals = E.cast_values()
    want = ref.trunc_to_int64(vals)
    src = E.device_array(vals, DEV)
    dst = E.guarded(vals.size, E.SENTINEL64, DEV)
    _lib.call("plato_agg_cast_f32_i64", src.data_ptr(), dst.data_ptr(), vals.size, _stream())
    torch.cuda.synchronize()
    got = E.fetch(dst, np.uint64)
    assert (got[vals.size:] == E.SENTINEL64).all(), "guard words overwritten"
    bad = np.nonzero(got[:vals.size].view(np.int64) != want)[0]
    assert bad.size == 0, (vals[bad[:5]], got[:vals.size].view(np.int64)[bad[:5]], want[bad[:5]])
    assert np.array_equal(cast_to_int64(torch.from_numpy(vals).to(DEV)).cpu().numpy(), want)


def _fill(kind: str, n: int, add, first, seed=11, stream_id=4):
    """plato_agg_fill_synth_<kind> (first is None) or ..._at on n elements; ``add``: a device pointer or None."""
    sentinel, last = (E.SENTINEL32, -30) if kind == "f32" else (E.SENTINEL64, 9)  # last: scale_log2 / modulus
    out = E.guarded(n, sentinel, DEV)
    if first is None:
        _lib.call(f"plato_agg_fill_synth_{kind}", out.data_ptr(), add, n, seed, stream_id, last, _stream())
    else:
        _lib.call(f"plato_agg_fill_synth_{kind}_at", out.data_ptr(), add, n, seed, stream_id, first, last, _stream())
    torch.cuda.synchronize()
    got = E.fetch(out, np.uint32 if kind == "f32" else np.uint64)
    assert (got[n:] == sentinel).all(), "guard words overwritten"
    return got[:n]


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("first", [0, 1, 255, 256, 1000])
def test_fill_synth_at_is_a_slice_of_the_whole_stream(first, n, with_add):
    for kind, item in (("f32", 4), ("i64", 8)):
        add = None
        if with_add:  # the addend of the whole stream; the slice gets its elements first .. first + n
            host = synth.synth_f32(first + n, 3, 0, -27) if kind == "f32" else synth.synth_i64(first + n, 3, 0, 10_001)
            add = E.device_array(host, DEV)
        whole = _fill(kind, first + n, None if add is None else add.data_ptr(), None)
        part = _fill(kind, n, None if add is None else add.data_ptr() + item * first, first)
        assert np.array_equal(whole[first:], part), kind


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
def test_fill_synth_at_across_32_bits(with_add):
    """first = 2^32 - 3, n = 8: the element index crosses 32 bits inside the slice; against oracle/synth.py."""
    first, n = 2**32 - 3, 8
    add_f = synth.synth_f32(n, 3, 0, -27) if with_add else None
    add_i = synth.synth_i64(n, 3, 0, 10_001) if with_add else None
    d_f = None if add_f is None else E.device_array(add_f, DEV)
    d_i = None if add_i is None else E.device_array(add_i, DEV)
    got = _fill("f32", n, None if d_f is None else d_f.data_ptr(), first)
    assert np.array_equal(got, synth.synth_f32(n, 11, 4, -30, add=add_f, start=first).view(np.uint32))
    got = _fill("i64", n, None if d_i is None else d_i.data_ptr(), first)
    assert np.array_equal(got.view(np.int64), synth.synth_i64(n, 11, 4, 9, add=add_i, start=first))
