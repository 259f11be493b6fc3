"""``plato_agg_decode_rows`` on the rows themselves.

The suite reached the decode kernel only through ``rnd.decoded()`` and the digest of a downstream
reduction.  Here the decoded rows are compared element by element with the host decode of the same
payloads (plato/processors/model_dequantize.py:15-18, model_dequantize_qsgd.py:34-60), for chunk tables
cut at 4, 256 and 4096 elements over a ragged layout (tests/edge_cases.py decode_layout), K = 1, 2, 5,
a non-zero ``i64_dst_offset``, and destination rows pre-filled with a sentinel: every position outside
the entries — the fp32 region's alignment padding, the gap before the int64 block, everything behind
it — must still hold the sentinel afterwards.
"""

import numpy as np
import pytest
import torch

from oracle import qsgd as Q
from plato_amd import _lib
from plato_amd.arena import ArenaLayout
from plato_amd.engine import FedAvgEngine
from tests import edge_cases as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYOUTS = {True: E.decode_layout(True), False: E.decode_layout(False)}


def device_decode(layout: ArenaLayout, codec: str, cap: int, src_f, src_i, mv, divisor: float) -> np.ndarray:
    """The K destination rows (uint32 bit patterns, guard included) after one plato_agg_decode_rows call."""
    k = len(src_f)
    n_i = layout.n_i64
    dst_off = layout.n_f32 + 37
    row_len = dst_off + n_i + E.GUARD
    keep_f, pf = E.device_rows(np.stack(src_f), DEV)
    keep_i, pi = E.device_rows(np.stack(src_i), DEV)
    dst = torch.from_numpy(np.full((k, row_len), E.SENTINEL32).view(np.int32)).to(DEV)
    tab = E.pointer_table(pf + pi + [dst.data_ptr() + 4 * row_len * r for r in range(k)], DEV)
    cf, ci = layout.chunk_tables(cap)
    dcf, dci = E.device_array(cf, DEV), E.device_array(ci, DEV)
    dmv = None if mv is None else E.device_array(mv, DEV)
    _lib.call("plato_agg_decode_rows", _lib.PLATO_AGG_DECODE[codec], tab.data_ptr(), tab.data_ptr() + 8 * k, k,
              None if dmv is None else dmv.data_ptr(), float(divisor), dcf.data_ptr(), int(cf.shape[0]),
              dci.data_ptr() if ci.shape[0] else None, int(ci.shape[0]), dst_off, tab.data_ptr() + 16 * k,
              torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(np.uint32)


def check_rows(layout, codec, cap, k, seed, divisor=0):
    src_f, src_i, mv = E.decode_sources(layout, codec, k, seed)
    got = device_decode(layout, codec, cap, src_f, src_i, mv, divisor)
    dst_off = layout.n_f32 + 37
    for c in range(k):
        vf, vi = E.decode_values(layout, codec, src_f[c], src_i[c], None if mv is None else mv[:, c], divisor)
        want = E.decode_expected_row(layout, vf, vi, dst_off, got.shape[1])
        # bf16 and native are exact copies / widenings: raw bits, NaN payloads and signs included
        row = E.bits32(got[c].view(np.float32)) if codec == "qsgd" else got[c]
        bad = np.nonzero(row != want)[0]
        assert bad.size == 0, (f"{codec} cap={cap} K={k} client {c}: {bad.size} positions differ, first at {bad[0]} "
                               f"(n_f32={layout.n_f32}, int64 block at {dst_off}): got {row[bad[0]]:#010x} "
                               f"want {want[bad[0]]:#010x}")


@pytest.mark.parametrize("with_i64", [True, False], ids=["i64", "f32only"])
@pytest.mark.parametrize("k", E.DECODE_KS)
@pytest.mark.parametrize("cap", E.DECODE_CAPS)
def test_bf16_rows_hold_every_pattern_widened_exactly(cap, k, with_i64):
    check_rows(LAYOUTS[with_i64], "bf16", cap, k, seed=cap + k)


@pytest.mark.parametrize("with_i64", [True, False], ids=["i64", "f32only"])
@pytest.mark.parametrize("k", E.DECODE_KS)
@pytest.mark.parametrize("cap", E.DECODE_CAPS)
def test_native_rows_copy_fp32_bits_and_round_int64_to_nearest_even(cap, k, with_i64):
    check_rows(LAYOUTS[with_i64], "native", cap, k, seed=cap + k)


@pytest.mark.parametrize("with_i64", [True, False], ids=["i64", "f32only"])
@pytest.mark.parametrize("divisor", E.QSGD_DIVISORS)
@pytest.mark.parametrize("k", E.DECODE_KS)
@pytest.mark.parametrize("cap", E.DECODE_CAPS)
def test_qsgd_rows_match_the_dequantizer(cap, k, divisor, with_i64):
    """Every code byte under every max_v of {0, 1e-45, 1.17e-38, 1e-3, 1, 3.4e38, inf, NaN} and the divisors
    1, 3, 127, 255, max_v laid out [n_entries][K] with a different value per (entry, client).  The reference
    is oracle.qsgd.dequantize_regions (pinned to the reference's fixtures by tests/test_qsgd.py), i.e. the
    fp32 chain

        zeta = -(byte - 128) if byte >= 128 else byte            (an integer: byte 128 is 0, not -0.0)
        x    = fp32(fp32(fp32(zeta) * max_v) / divisor)

    with one rounding per operation: the product may overflow to +-inf before the division, 0 * inf and
    any NaN max_v give NaN, and a subnormal quotient (1e-45 or 1.17e-38 over 3, 127, 255) is kept, not
    flushed to zero."""
    check_rows(LAYOUTS[with_i64], "qsgd", cap, k, seed=divisor + k, divisor=divisor)


def test_decode_rows_refusals_on_the_device():
    """Refused calls and the empty call leave the destination rows untouched."""
    layout = LAYOUTS[True]
    src_f, src_i, mv = E.decode_sources(layout, "qsgd", 1, 0)
    keep_f, pf = E.device_rows(np.stack(src_f), DEV)
    keep_i, pi = E.device_rows(np.stack(src_i), DEV)
    row_len = layout.n_f32 + layout.n_i64 + E.GUARD
    dst = torch.from_numpy(np.full((1, row_len), E.SENTINEL32).view(np.int32)).to(DEV)
    tab = E.pointer_table(pf + pi + [dst.data_ptr()], DEV)
    cf, ci = layout.chunk_tables(4096)
    dcf, dci, dmv = E.device_array(cf, DEV), E.device_array(ci, DEV), E.device_array(mv, DEV)
    h = torch.cuda.current_stream(DEV).cuda_stream

    def call(codec, k, max_v, divisor, ncf, nci):
        _lib.call("plato_agg_decode_rows", codec, tab.data_ptr(), tab.data_ptr() + 8, k, max_v, divisor,
                  dcf.data_ptr(), ncf, dci.data_ptr(), nci, layout.n_f32, tab.data_ptr() + 16, h)

    ncf, nci = int(cf.shape[0]), int(ci.shape[0])
    for k in (0, 65536):
        with pytest.raises(ValueError, match="K must be"):
            call(2, k, dmv.data_ptr(), 63.0, ncf, nci)
    for codec in (-1, 3):
        with pytest.raises(ValueError, match="bad codec"):
            call(codec, 1, dmv.data_ptr(), 63.0, ncf, nci)
    with pytest.raises(ValueError, match="QSGD needs"):
        call(2, 1, None, 63.0, ncf, nci)
    with pytest.raises(ValueError, match="QSGD needs"):
        call(2, 1, dmv.data_ptr(), 0.0, ncf, nci)
    call(2, 1, dmv.data_ptr(), 63.0, 0, 0)  # no chunks: success without a launch
    torch.cuda.synchronize()
    assert bool((dst.view(torch.int32) == int(np.int32(np.uint32(E.SENTINEL32).view(np.int32)))).all())


def _engine_payloads(codec: str, seed: int):
    """One layout of tests/test_fuzz_variants_gpu._spec with K coded payloads and their host decode."""
    from plato_amd.processors.qsgd import Processor
    from tests.test_fuzz_variants_gpu import _spec

    spec, k = _spec(seed)
    # the QSGD wire header holds each dimension as a big-endian int16
    spec = [(n, (8, -(-shape[0] // 8)) if len(shape) == 1 and shape[0] > 32767 else shape, r) for n, shape, r in spec]
    layout = ArenaLayout.from_shapes(spec)
    rng = np.random.default_rng(seed)
    bf = (rng.standard_normal(layout.n_f32) * 0.05).astype(np.float32)
    bi = rng.integers(-(1 << 40), 1 << 40, layout.n_i64)
    baseline = layout.unpack(torch.from_numpy(bf), torch.from_numpy(bi))
    payloads, decoded = [], []
    if codec == "bf16":
        for _ in range(k):
            bits_f = rng.integers(0, 1 << 16, layout.n_f32).astype(np.uint16)
            bits_i = rng.integers(0, 1 << 16, layout.n_i64).astype(np.uint16)
            sd = layout.unpack(torch.from_numpy(bits_f.view(np.int16)).view(torch.bfloat16),
                               torch.from_numpy(bits_i.view(np.int16)).view(torch.bfloat16))
            payloads.append(sd)
            decoded.append(((bits_f.astype(np.uint32) << 16), (bits_i.astype(np.uint32) << 16)))
    else:
        level = 64
        proc = Processor(quantization_level=level)
        for _ in range(k):
            cf = rng.integers(0, 256, layout.n_f32).astype(np.uint8)
            ci = rng.integers(0, 256, layout.n_i64).astype(np.uint8)
            mv = rng.uniform(0.01, 3.0, len(layout.entries)).astype(np.float32)
            wire = {e.name: Q.encode_layer((cf if e.region == "f32" else ci)[e.offset:e.offset + e.numel], mv[e_i],
                                           e.shape) for e_i, e in enumerate(layout.entries)}
            payloads.append(proc.process(wire))
            vf, vi = Q.dequantize_regions(layout.entries, cf, ci, mv, level)
            decoded.append((E.bits32(vf), E.bits32(vi)))
    return layout, k, bf, bi, baseline, payloads, decoded


@pytest.mark.parametrize("codec,seed", [("bf16", 3), ("qsgd", 4)])
def test_engine_decoded_rows_equal_the_host_decode(codec, seed):
    layout, k, bf, bi, baseline, payloads, decoded = _engine_payloads(codec, seed)
    engine = FedAvgEngine(DEV)
    rnd = engine.begin(baseline, k, codec)
    rnd.put_baseline(baseline)
    for slot, p in enumerate(payloads):
        rnd.put_client(slot, p)
    work = rnd.decoded()
    assert rnd.decoded() is work and work.decoded() is work  # decoded once per staged set
    torch.cuda.synchronize()
    play = work.layout
    assert play.n_i64 == 0 and [e.name for e in play.entries] == [e.name for e in layout.entries]
    rows = work.slab.f32.cpu().numpy().view(np.uint32)
    base_row = work._base.f32.cpu().numpy().view(np.uint32)
    want_base = (bf.view(np.uint32), bi.astype(np.float32).view(np.uint32))
    for e, pe in zip(layout.entries, play.entries):
        region = 0 if e.region == "f32" else 1
        assert pe.offset == (e.offset if region == 0 else layout.row_f32 + e.offset)
        sl, psl = slice(e.offset, e.offset + e.numel), slice(pe.offset, pe.offset + pe.numel)
        assert np.array_equal(base_row[psl], want_base[region][sl]), e.name
        for slot in range(k):
            got = rows[slot, psl]
            if codec == "qsgd":
                got = E.bits32(got.view(np.float32))
            assert np.array_equal(got, decoded[slot][region][sl]), (e.name, slot)


def test_native_round_decodes_to_itself():
    layout = ArenaLayout.from_shapes([("a", (5,), "f32"), ("n", (), "i64")])
    base = layout.unpack(torch.zeros(5), torch.zeros(1, dtype=torch.int64))
    rnd = FedAvgEngine(DEV).begin(base, 1)
    assert rnd.decoded() is rnd
