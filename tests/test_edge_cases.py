"""The case generators and host references of tests/edge_cases.py, run without a device, and the
conditions the GPU comparisons built on them rest on: the exact-input dot products stay below 2^53, the
special-value seeds of the float64-weight sweep leave most outputs comparable, the base mode of
``w64_numpy`` is the composition it claims, and the synthetic streams' starting offset is a slice."""

import math

import numpy as np
import pytest

from oracle import qsgd as Q
from oracle import synth
from tests import edge_cases as E


def test_sweeps_hold_the_unroll_edges():
    assert {E.K_SU - 1, E.K_SU, E.K_SU + 1} <= set(E.W64_KS) and {1, 2, 3, 4, 5, 7, 8, 9, 16, 17} <= set(E.W64_KS)
    assert len(E.W64_SHAPES) == len(E.W64_NF) * len(E.W64_NI) - 1 and (0, 0) not in E.W64_SHAPES
    assert (3, 300) in E.W64_SHAPES  # 303 scalar items: the second scalar workgroup
    seeds = [E.w64_seed(k, i) for k in E.W64_KS for i in range(len(E.W64_SHAPES))]
    assert len(set(seeds)) == len(seeds)
    # every weight the sweep must hold occurs in some case, and w_i64 never equals the cast of w64
    seen = set()
    nan_weights = 0
    for k in E.W64_KS:
        for i in (0, 5, 17, 30):
            c = E.w64_case(k, 5, 1, E.w64_seed(k, i))
            seen.update(np.float64(w).tobytes() for w in c["w64"])
            nan_weights += any(math.isnan(w) for w in c["w64"])
            assert sorted(c["order"]) == list(range(k))
            with np.errstate(over="ignore"):
                assert [np.float32(w) for w in c["w64"]] != [np.float32(w) for w in c["w_i64"]]
    for w in E.HARD_W64:
        assert np.float64(w).tobytes() in seen, w
    assert nan_weights > 0


@pytest.mark.parametrize("k", E.W64_KS)
def test_w64_special_seeds_stay_comparable_and_base_mode_is_the_composition(k):
    """NaN share < 50 % of the reference's outputs in every special-value seed (both modes), and
    w64_numpy(x, base) == update(b, w64_numpy(x - b)) bit for bit on every case of the sweep."""
    specials = 0
    for i, (n_f, n_i) in enumerate(E.W64_SHAPES):
        if n_f > 2000 and i % 2:  # the long arenas: every other case is enough on the CPU
            continue
        c = E.w64_case(k, n_f, n_i, E.w64_seed(k, i))
        with_base = E.w64_reference(c, True)
        comp = E.w64_composed(c)
        assert E.bits32(with_base[0]).tobytes() == E.bits32(comp[0]).tobytes(), (k, n_f, n_i)
        assert E.bits32(with_base[1]).tobytes() == E.bits32(comp[1]).tobytes(), (k, n_f, n_i)
        if c["special"]:
            specials += 1
            assert E.nan_share(*with_base) < 0.5, (k, n_f, n_i)
            assert E.nan_share(*E.w64_reference(c, False)) < 0.5, (k, n_f, n_i)
            planted = sum(int(np.isin(a.view(np.uint32), E.SPECIAL_F32.view(np.uint32)).sum())
                          for a in (c["base_f"], c["xs_f"]))
            assert planted > 0 or n_f * (k + 1) < 200
    assert specials >= 10


def test_w64_wrapping_differences_occur():
    c = E.w64_case(5, 5, 300, 3)
    assert c["special"]
    wide = c["xs_i"].astype(object) - c["base_i"].astype(object)[None, :]
    assert (np.abs(wide) > 2**63).any()  # the true difference does not fit: the int64 one wraps


def test_f64_reference_is_the_sequential_loop():
    xs, w = E.f64_case(5, 257, 1)
    acc = [0.0] * 257
    for i in range(5):
        with np.errstate(all="ignore"):
            acc = [np.float64(a) + np.float64(x) * np.float64(w[i]) for a, x in zip(acc, xs[i])]
    assert E.bits64(np.asarray(acc)).tobytes() == E.bits64(E.f64_reference(xs, w)).tobytes()
    # the sweep holds the specials somewhere, and small n too
    pool = set()
    for n in E.F64_NS[:6]:
        for k in E.F64_KS:
            xs, w = E.f64_case(k, n, 7 * k + n)
            pool.update(xs.view(np.uint64).reshape(-1).tolist())
    for s in E.SPECIAL_F64.view(np.uint64):
        assert int(s) in pool


@pytest.mark.parametrize("with_i64", [True, False])
def test_decode_layout_and_references(with_i64):
    lay = E.decode_layout(with_i64)
    sizes = [e.numel for e in lay.entries if e.region == "f32"]
    assert sizes[:7] == [0, 1, 5, 255, 256, 257, 5000] and max(sizes) >= 1 << 16
    if with_i64:
        regions = [e.region for e in lay.entries]
        assert regions[0] == "i64" and regions[-1] == "i64" and lay["c3"].numel == 3
        assert lay["c_mid"].numel == 1 and lay.n_i64 >= 1 << 16
    else:
        assert lay.n_i64 == 0 and not lay.packed  # padding inside the fp32 region
    for cap in E.DECODE_CAPS:
        cf, ci = lay.chunk_tables(cap)
        lens = (cf[:, 2] - cf[:, 1]).astype(np.int64)
        assert lens.max() <= cap and int(lens.sum()) == sum(sizes)
        assert (lens < 256).any() and ((lens == 256).any() or cap < 256) and ((lens > 256).any() or cap <= 256)
    k = 2
    # bf16: every pattern in each region of each client; the widening keeps every bit
    sf, si, _ = E.decode_sources(lay, "bf16", k, 1)
    for c in range(k):
        for e in lay.entries:
            if e.numel >= 1 << 16:
                src = sf[c] if e.region == "f32" else si[c]
                assert np.unique(src[e.offset:e.offset + e.numel]).size == 1 << 16
    vf, vi = E.decode_values(lay, "bf16", sf[0], si[0], None, 0)
    assert np.array_equal((vf >> 16).astype(np.uint16), sf[0]) and not (vf & 0xFFFF).any()
    # QSGD: every (byte, max_v) pair, max_v different per (entry, client), and the written-out chain
    for divisor in E.QSGD_DIVISORS:
        sf, si, mv = E.decode_sources(lay, "qsgd", k, divisor)
        assert mv.shape == (len(lay.entries), k) and np.unique(E.bits32(mv)).size > mv.size // 2
        vf, vi = E.decode_values(lay, "qsgd", sf[1], si[1], mv[:, 1], divisor)
        for e_i, e in enumerate(lay.entries):
            codes = (sf[1] if e.region == "f32" else si[1])[e.offset:e.offset + e.numel]
            got = (vf if e.region == "f32" else vi)[e.offset:e.offset + e.numel]
            assert np.array_equal(got, E.bits32(E.qsgd_chain(codes, mv[e_i, 1], divisor))), e.name
    pairs = set()
    for seed in range(8):
        sf, si, mv = E.decode_sources(lay, "qsgd", 1, seed)
        for e_i, e in enumerate(lay.entries):
            if e.name.startswith("q"):
                codes = (sf[0] if e.region == "f32" else si[0])[e.offset:e.offset + e.numel]
                assert sorted(codes.tolist()) == list(range(256))
                pairs.add(int(E.bits32(mv[e_i:e_i + 1, 0])[0]))
    assert len(pairs) == len(E.QSGD_MAX_V)
    # native: RNE at the ties and the extremes, as numpy casts
    sf, si, _ = E.decode_sources(lay, "native", k, 2)
    if with_i64:
        vf, vi = E.decode_values(lay, "native", sf[0], si[0], None, 0)
        at = lay["cbig"].offset
        want = np.array([0, 1, -1, 2.0**24, -(2.0**24), 2.0**24 + 4, -(2.0**24 + 4), 2.0**53, -(2.0**63), 2.0**63],
                        dtype=np.float32)
        assert np.array_equal(vi[at:at + want.size], want.view(np.uint32))
        assert np.isnan(sf[0]).any()
    # the expected row: the sentinel in the gap, behind the int64 block and in the fp32 region's padding
    vf, vi = E.decode_values(lay, "native", sf[0], si[0], None, 0)
    off = lay.n_f32 + 37
    row = E.decode_expected_row(lay, vf, vi, off, off + lay.n_i64 + E.GUARD)
    assert (row[lay.n_f32:off] == E.SENTINEL32).all() and (row[off + lay.n_i64:] == E.SENTINEL32).all()
    touched = sum(e.numel for e in lay.entries)
    assert int((row != E.SENTINEL32).sum()) >= touched - 4  # a random pattern may equal the sentinel
    if not with_i64:
        assert int((row[:lay.n_f32] == E.SENTINEL32).sum()) >= lay.n_f32 - lay.n_f32_data


def test_qsgd_chain_cases_to_watch():
    """Byte 128 is -0 -> integer 0 -> +0.0 before the multiply; the subnormal quotients are kept."""
    codes = np.array([128, 0, 1, 129, 127, 255], dtype=np.uint8)
    out = E.qsgd_chain(codes, np.float32(1.0), 3)
    assert out.view(np.uint32)[0] == 0 and out.view(np.uint32)[1] == 0
    assert out[2] == np.float32(1.0) / np.float32(3.0) and out[3] == -out[2]
    tiny = E.qsgd_chain(codes, np.float32(1.17e-38), 127)
    assert tiny[4] != 0 and abs(tiny[4]) < np.finfo(np.float32).tiny  # a subnormal quotient, not flushed
    blob = Q.encode_layer(codes, 1.17e-38, (6,))
    assert np.array_equal(Q.decode_layer(blob, 128).view(np.uint32), tiny.view(np.uint32))


@pytest.mark.parametrize("has_base", [False, True])
@pytest.mark.parametrize("k", E.DOTS_KS)
def test_dots_exact_inputs_stay_below_2_53(k, has_base):
    seed = 0
    for n_f in E.DOTS_NF:
        for n_i in E.DOTS_NI:
            seed += 1
            if n_f > 5000 and n_i != 5:
                continue
            c = E.dots_case("exact", k, n_f, n_i, has_base, 1000 * k + seed)
            out, abs_sum = E.dots_reference_exact(c)
            assert abs_sum < 2**53 and len(out) == 2 * k + 1
            d, v = E.dots_vectors(c)
            # the integers are what the fp64 sums of the fp32 values are, in numpy's order for one
            assert float(out[0]) == float(np.dot(d[0].astype(np.float64), v.astype(np.float64)))
            if n_f + n_i:
                assert out[-1] > 0 or not v.any()


def test_dots_general_reference_and_bound():
    c = E.dots_case("general", 9, 1027, 5, True, 5, wrap=True)
    d, v = E.dots_vectors(c)
    # the wrapping differences: fp32 of the wrapped int64, not of the true difference
    assert d[0, 1027] == np.float32(-(2.0**63) + 1) and d[0, 1028] == np.float32(-(2.0**63) + 5)
    c = E.dots_case("general", 9, 1027, 5, True, 5)
    d, v = E.dots_vectors(c)
    ref_out, bound = E.dots_reference_general(c)
    assert ref_out.shape == bound.shape == (19,) and (bound > 0).all()
    # numpy's own fp64 dot (pairwise / blocked order) is one of the orders the bound covers
    for i in range(9):
        assert abs(np.dot(d[i].astype(np.float64), v.astype(np.float64)) - ref_out[i]) <= bound[i]
        assert abs(np.dot(d[i].astype(np.float64), d[i].astype(np.float64)) - ref_out[9 + i]) <= bound[9 + i]
    # and the bound is tight enough to see one dropped element
    assert (np.abs(d[:, 1026].astype(np.float64) * v[1026]) > bound[:9]).any()
    empty = E.dots_reference_general(E.dots_case("general", 1, 0, 0, False, 1))
    assert empty[0].tolist() == [0.0, 0.0, 0.0] and empty[1].tolist() == [0.0, 0.0, 0.0]


def test_cast_values_hold_the_boundaries():
    vals = E.cast_values()
    assert vals.size == 4096 + 2 * 277 + 6
    edge = np.float32(2.0**63)
    for x in (edge, -edge, np.float32(2.0**-149), np.float32(-(2.0**127)), np.nextafter(edge, np.float32(0)),
              np.nextafter(-edge, np.float32(-np.inf))):
        assert (vals == x).any()
    from oracle import fedavg_oracle as ref

    out = ref.trunc_to_int64(np.array([np.nextafter(edge, np.float32(0)), edge, -edge,
                                       np.nextafter(-edge, np.float32(-np.inf))], dtype=np.float32))
    assert out.tolist() == [2**63 - 2**39, -2**63, -2**63, -2**63]


@pytest.mark.parametrize("first", [0, 1, 255, 256, 1000])
def test_synth_offset_is_a_slice_of_the_stream(first):
    n, seed, stream = 257, 11, 4
    add_f = synth.synth_f32(first + n, seed, 0, synth.BASE_SCALE)
    add_i = synth.synth_i64(first + n, seed, 0, synth.I64_BASE_MOD)
    for add in (None, add_f):
        whole = synth.synth_f32(first + n, seed, stream, synth.CLIENT_SCALE, add=add)
        part = synth.synth_f32(n, seed, stream, synth.CLIENT_SCALE, add=None if add is None else add[first:],
                               start=first)
        assert whole[first:].tobytes() == part.tobytes()
    for add in (None, add_i):
        whole = synth.synth_i64(first + n, seed, stream, 9, add=add)
        part = synth.synth_i64(n, seed, stream, 9, add=None if add is None else add[first:], start=first)
        assert np.array_equal(whole[first:], part)
    if first == 0:  # the argument's default is the stream from its beginning
        assert synth.synth_f32(n, seed, stream, -30).tobytes() == synth.synth_f32(n, seed, stream, -30, start=0).tobytes()
        assert np.array_equal(synth.synth_i64(n, seed, stream, 9), synth.synth_i64(n, seed, stream, 9, start=0))


def test_synth_offset_across_32_bits_is_the_scalar_generator():
    first, n, seed, stream = 2**32 - 3, 8, 11, 4
    key = synth.synth_key(seed, stream)
    hs = [synth.splitmix64_int((key + first + e) & ((1 << 64) - 1)) for e in range(n)]
    want_i = [h % 10_001 for h in hs]
    assert synth.synth_i64(n, seed, stream, 10_001, start=first).tolist() == want_i
    want_f = [np.float32(((h >> 40) - (1 << 23)) * 2.0**-27) for h in hs]
    assert synth.synth_f32(n, seed, stream, -27, start=first).tolist() == want_f
    # elements 3.. lie past 2^32: an offset kept in 32 bits would restart the stream there
    assert want_i[3:] != synth.synth_i64(n - 3, seed, stream, 10_001, start=0).tolist()
