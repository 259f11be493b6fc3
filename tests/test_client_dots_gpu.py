"""``plato_agg_client_dots`` (+ ``_workspace``): the model-wide fp64 reductions d_i.v, |d_i|^2, |v|^2.

The kernel accumulates in fp64 in a fixed order of its own, so it is bit-equal to no host order in
general.  Two kinds of input pin it all the same (tests/edge_cases.py):

* exact inputs — small integers, every product and every partial sum an exact double (sums below
  2^53, asserted from the reference): the 2K+1 outputs must EQUAL the integer sums, whatever the
  order.  A dropped tail, a double-counted clamped client of the 8-client batch, a wrong base or a
  missing int64 term fails with no tolerance at all;
* general inputs — standard-normal values against ``math.fsum`` of the exact products, within the
  derived bound ``n * 2^-52 * fsum(|t_i|)`` (edge_cases.dots_reference_general).

K at the edges of the 8-client batch, fp32 arenas of 0 to 300,003 elements (every float4 tail; more than
256 chunk partials, so dots_final's strided loop runs twice), 0 / 1 / 5 int64 entries, with and without
a base, guard doubles behind the outputs and the workspace, and two calls that must agree byte for byte.
"""

import numpy as np
import pytest
import torch

from plato_amd import _lib
from tests import edge_cases as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def device_dots(c: dict) -> np.ndarray:
    return E.device_dots(c, DEV)


def _shapes():
    return [(n_f, n_i) for n_f in E.DOTS_NF for n_i in E.DOTS_NI]


@pytest.mark.parametrize("has_base", [False, True], ids=["raw", "base"])
@pytest.mark.parametrize("k", E.DOTS_KS)
def test_exact_inputs_give_the_integer_sums(k, has_base):
    for i, (n_f, n_i) in enumerate(_shapes()):
        c = E.dots_case("exact", k, n_f, n_i, has_base, 100 * k + i)
        want, abs_sum = E.dots_reference_exact(c)
        assert abs_sum < 2**53  # every partial sum, in any order, is an exact double
        got = device_dots(c)
        assert got.tolist() == [float(x) for x in want], (k, n_f, n_i, has_base)


@pytest.mark.parametrize("n_i", E.DOTS_NI)
@pytest.mark.parametrize("has_base", [False, True], ids=["raw", "base"])
@pytest.mark.parametrize("k", E.DOTS_KS)
def test_general_inputs_stay_within_the_derived_bound(k, has_base, n_i):
    for i, n_f in enumerate(E.DOTS_NF):
        c = E.dots_case("general", k, n_f, n_i, has_base, 1000 * k + 10 * i + n_i)
        want, bound = E.dots_reference_general(c)
        got = device_dots(c)
        err = np.abs(got - want)
        assert (err <= bound).all(), (k, n_f, n_i, has_base, int(np.argmax(err - bound)), err.max(), bound.min())


def test_wrapping_int64_differences():
    c = E.dots_case("general", 9, 1027, 5, True, 77, wrap=True)
    want, bound = E.dots_reference_general(c)
    got = device_dots(c)
    assert (np.abs(got - want) <= bound).all()
    assert (got[9:18] > 2.0**125).all()  # (2^63)^2 is in every |d_i|^2: the difference wrapped, then was cast


def test_client_dots_refusals_on_the_device():
    c = E.dots_case("exact", 2, 5, 1, True, 1)
    keep_f, pf = E.device_rows(c["x"], DEV)
    keep_i, pi = E.device_rows(c["xi"], DEV)
    tf, ti = E.pointer_table(pf, DEV), E.pointer_table(pi, DEV)
    b, bi, v, vi = (E.device_array(c[n], DEV) for n in ("b", "bi", "v", "vi"))
    ws = E.guarded(8, E.SENTINEL64, DEV)
    out = E.guarded(5, E.SENTINEL64, DEV)
    h = torch.cuda.current_stream(DEV).cuda_stream
    ok = [tf.data_ptr(), ti.data_ptr(), 2, b.data_ptr(), bi.data_ptr(), v.data_ptr(), vi.data_ptr(), 5, 1,
          ws.data_ptr(), out.data_ptr(), h]

    def refused(match, **change):
        args = list(ok)
        for pos, value in change.items():
            args[int(pos[1:])] = value
        with pytest.raises(ValueError, match=match):
            _lib.call("plato_agg_client_dots", *args)

    refused("K must be", a2=0)
    for pos in ("a0", "a5", "a9", "a10"):  # d_x, d_v, d_workspace, d_out
        refused("null", **{pos: None})
    for pos in ("a1", "a6", "a4"):  # the int64 pointers with n_i64 > 0 (a4: a base without its int64 half)
        refused("null int64", **{pos: None})
    refused("aligned", a5=v.data_ptr() + 4)
    refused("aligned", a3=b.data_ptr() + 4)
    torch.cuda.synchronize()
    assert (E.fetch(out, np.uint64) == E.SENTINEL64).all() and (E.fetch(ws, np.uint64) == E.SENTINEL64).all()
