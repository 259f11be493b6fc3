"""Float32 division by a float64 reciprocal product: x / d computed as
float32(float64(x) * (1 / float64(d))) (the FedAdp producers' division by -lr, fedadp.hip adp_div_lr_f64,
and the QSGD decode tables, qsgd.hip decode_tab / decode_arith) gives the float32 division's bits for
every x, including subnormals, zeros, infinities and overflow to infinity, when the divisor is not an
even integer, or is a power of two (csrc/common.h recip_product_exact, restated below).

For any other divisor, an even integer d that is no power of two, the identity can fail, and only at a
quotient that is exactly a tie between two float32 subnormals, an odd multiple of 2^-150: the dividend
p = (2m + 1) * (d / 2) * 2^-149 is then a float, IEEE division rounds the tie to even, and the float64
product, computed with an inexact reciprocal, lands beside the tie and rounds to the nearer neighbour.
Worked case: d = 98, p = 147 * 2^-149: the quotient is 3 * 2^-150, division gives 2^-148 (bits 0x2), the
product 2^-149 (bits 0x1).  The kernels therefore take the product only for a safe divisor and the IEEE
division otherwise (run_qsgd, adp_for_lr)."""

import struct

import numpy as np
import pytest

from oracle import qsgd as Q

TINY = np.float64(2.0**-149)  # the smallest float32 subnormal


def recip_product_exact(d) -> bool:
    """csrc/common.h recip_product_exact: safe iff d is not an even integer, or |d| is a power of two."""
    a = abs(float(np.float32(d)))
    if not (a >= 2.0) or np.isinf(a):  # no even integer below 2 (NaN: both forms give NaN)
        return True
    if np.frexp(a)[0] == 0.5:
        return True
    return a % 2.0 != 0.0


def _division(p: np.ndarray, d) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.divide(p, np.float32(d), dtype=np.float32)


def _product(p: np.ndarray, d) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (p.astype(np.float64) * (1.0 / np.float64(np.float32(d)))).astype(np.float32)


def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("lr", [0.01, 0.1, 1.0, 3e-5, 0.37, 7.3e-39, 1e30, -0.05])
def test_f64_reciprocal_product_rounds_like_f32_division(lr):
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2**32, size=2_000_000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = np.concatenate([v[np.isfinite(v)], np.array([0.0, -0.0, 1e-45, -1e-45, 3.4e38], np.float32)])
    lr32 = np.float32(lr)
    with np.errstate(all="ignore"):
        want = v / lr32
        got = (v.astype(np.float64) * (1.0 / np.float64(lr32))).astype(np.float32)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))


def test_f64_reciprocal_product_rounds_like_f32_division_random_divisors():
    """Random divisors over the whole float32 range (signs, subnormals, zero and infinity included),
    random dividends: the identity for any learning rate, not only the sampled ones above."""
    rng = np.random.default_rng(11)
    dbits = rng.integers(0, 2**32, size=400, dtype=np.uint64).astype(np.uint32)
    ds = dbits.view(np.float32)
    ds = np.concatenate([ds[np.isfinite(ds)], np.array([1e-45, 1.17549435e-38, 1.0, 3.4e38, 0.0, np.inf],
                                                       np.float32)])
    for d in ds:
        bits = rng.integers(0, 2**32, size=50_000, dtype=np.uint64).astype(np.uint32)
        v = bits.view(np.float32)
        v = np.concatenate([v[~np.isnan(v)], np.array([0.0, -0.0, 1e-45, -3.4e38, np.inf], np.float32)])
        with np.errstate(all="ignore"):
            want = v / np.float32(d)
            got = (v.astype(np.float64) * (1.0 / np.float64(d))).astype(np.float32)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), d
        assert np.array_equal(want[~nan].view(np.uint32), got[~nan].view(np.uint32)), d


def test_safety_rule_classes():
    """The rule itself: even integers that are no power of two are the only unsafe divisors."""
    unsafe = [d for d in range(1, 256) if not recip_product_exact(d)]
    assert unsafe == [d for d in range(6, 256, 2) if d & (d - 1)]
    for d in (0.0, -0.0, 0.5, 1.0, 1.5, -1.999, 2.0, -2.0, 3.0, 4.0, 63.0, 97.5, 98.5, 128.0, 2.0**24, 2.0**100,
              np.inf, -np.inf, np.nan, 1e-45, 0.03):
        assert recip_product_exact(d), d
    for d in (6.0, -6.0, 98.0, -98.0, 196.0, 246.0, 2046.0, 3.0 * 2.0**24, 1e30):
        assert not recip_product_exact(d), d


def _tie_dividends(d: float, ms: np.ndarray) -> np.ndarray:
    """Every float whose quotient by d is the odd multiple (2m + 1) of 2^-150: p = (2m + 1) * (d / 2) * 2^-149,
    a float when d is an even integer.  For any other d no float has that quotient; the floats on both sides
    of (2m + 1) * (d / 2) * 2^-149 are returned instead (the dividends nearest to a tie)."""
    n = (2.0 * ms + 1.0) * (abs(float(d)) / 2.0)
    n = np.unique(np.concatenate([np.floor(n), np.ceil(n)]))
    n = n[n < 2.0**24]
    return (n * TINY).astype(np.float32)


def test_constructed_subnormal_ties():
    """Dividends built to put the quotient on (or as near as a float can get to) a tie between two
    subnormals, and every dividend n * 2^-149 with n < 2^16, both signs: for every divisor the rule calls
    safe the product has the division's bits; the worked case (d = 98, p = 147 * 2^-149) differs, so the
    sweep does reach the failure the rule exists for."""
    rng = np.random.default_rng(23)
    below2 = np.concatenate([
        np.array([0.01, 0.03, 0.1, 0.37, 0.5, 1.0, 1.5, 1.999, 3e-5, 7.3e-39, 1e-45], np.float32),
        rng.uniform(0.0, 2.0, 40).astype(np.float32),
        (2.0 ** rng.uniform(-20, 1, 40)).astype(np.float32)])
    below2 = below2[np.abs(below2) < 2]
    divisors = [float(d) for d in range(1, 256)] + [float(x) for x in below2] + [float(d) for d in range(2, 2049, 2)]
    ms = np.arange(4096, dtype=np.float64)
    dense = (np.arange(1 << 16, dtype=np.float64) * TINY).astype(np.float32)
    disagree = []
    for d in divisors:
        for sign in (1.0, -1.0):
            p = np.concatenate([_tie_dividends(d, ms), dense])
            want, got = _bits(_division(p, sign * d)), _bits(_product(p, sign * d))
            if recip_product_exact(d):
                bad = np.flatnonzero(want != got)
                assert bad.size == 0, (d, sign, p[bad[:4]], want[bad[:4]], got[bad[:4]])
            elif sign > 0 and not np.array_equal(want, got):
                disagree.append(d)
    worked = np.array([147.0 * TINY], np.float32)
    assert _bits(_division(worked, 98)).tolist() == [2]
    assert _bits(_product(worked, 98)).tolist() == [1]
    assert 98.0 in disagree
    # every divisor that disagrees is one the rule routes to the IEEE division
    assert all(not recip_product_exact(d) for d in disagree)
    # no learning rate below 2 can disagree
    assert min(disagree) >= 2
    # the rule is conservative: in the dense range alone only these divisors up to 255 reach a wrong tie
    # (6, 10, 254, ... do not), all even and none a power of two
    dense_bad = [d for d in range(1, 256) if not np.array_equal(_bits(_division(dense, d)), _bits(_product(dense, d)))]
    assert dense_bad == [98, 150, 154, 182, 186, 196, 198, 206, 210, 214, 234, 246]


def _two_step(zeta: np.ndarray, max_v: np.ndarray) -> np.ndarray:
    """p = fp32(fp32(zeta) * max_v), [len(max_v), len(zeta)]."""
    with np.errstate(all="ignore"):
        return np.multiply(zeta.astype(np.float32)[None, :], max_v.astype(np.float32)[:, None], dtype=np.float32)


def _decode_layer_values(max_v: np.float32, level: int) -> np.ndarray:
    """oracle.qsgd.decode_layer on the codes 0..127 under one max_v."""
    return Q.decode_layer(Q.encode_layer(np.arange(128, dtype=np.uint8), max_v, (128,)), level)


def test_qsgd_two_step_decode_follows_the_rule():
    """The kernels' table entry for |zeta| = 0..127: p = fp32(fp32(zeta) * max_v), then the float64 product
    for a safe divisor and the IEEE division otherwise, against oracle.qsgd.decode_layer's arithmetic
    (fp32(p / fp32(level - 1))) for every level 2..256, with max_v over the subnormals m * 2^-149, the tie
    makers of the level and small normals whose products straddle the subnormal range of the quotient."""
    rng = np.random.default_rng(29)
    zeta = np.arange(128)
    sub = (np.arange(1 << 11, dtype=np.float64) * TINY).astype(np.float32)
    normals = (2.0 ** rng.uniform(-126, -110, 512)).astype(np.float32)
    for level in range(2, 257):
        d = float(level - 1)
        max_v = np.concatenate([sub, _tie_dividends(d, np.arange(256, dtype=np.float64)), normals,
                                np.array([d * 2.0**-126, d * 2.0**-126 / 64, d * 2.0**-126 / 127], np.float32)])
        p = _two_step(zeta, max_v)
        want = _bits(_division(p, d))
        got = _bits(_product(p, d) if recip_product_exact(d) else _division(p, d))
        bad = np.argwhere(want != got)
        assert bad.size == 0, (level, bad[:4])
    # the vectorised model above is decode_layer's arithmetic: the oracle itself on a few max_v per level
    for level in (2, 7, 64, 99, 129, 151, 197, 247, 256):
        for mv in (np.float32(147 * TINY), np.float32(3e-39), np.float32(1.1754944e-38), np.float32(0.37)):
            p = _two_step(zeta, np.array([mv], np.float32))
            assert _bits(_decode_layer_values(mv, level)).tolist() == _bits(_division(p, level - 1))[0].tolist()
    # the wire format holds max_v as a float32: the worked case survives it and decodes to 2^-148 at code 1
    mv = struct.unpack("!f", struct.pack("!f", float(np.float32(147 * TINY))))[0]
    assert _bits(_decode_layer_values(np.float32(mv), 99))[1] == 2
    # and the product form, had it been kept for the unsafe levels, is wrong there: the entries the issue
    # counted for max_v = m * 2^-149, m < 2^14, zeta = 1..127
    sub14 = (np.arange(1 << 14, dtype=np.float64) * TINY).astype(np.float32)
    for d, count in ((98, 7370), (196, 8583)):
        p = _two_step(zeta[1:], sub14)
        assert int((_bits(_division(p, d)) != _bits(_product(p, d))).sum()) == count, d


def test_compiled_rule_matches_the_restatement(tmp_path):
    """csrc/common.h recip_product_exact itself, compiled into a small host program, against the Python
    restatement every test above uses: the integers 0..2049, halves, powers of two, huge and tiny floats,
    both signs, infinities and NaN."""
    import os
    import subprocess

    import __graft_entry__ as entry

    src = tmp_path / "rule.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "common.h"\n'
                   "int main(int argc, char** argv) {\n"
                   "  for (int i = 1; i < argc; ++i)\n"
                   "    std::putchar(plato_agg_internal::recip_product_exact(std::strtof(argv[i], nullptr)) ? '1' : '0');\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "rule"
    subprocess.run([entry._hipcc(), "-std=c++17", "-I", os.path.join(entry.PKG, "csrc"), "-I",
                    os.path.join(entry.ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rng = np.random.default_rng(31)
    ds = [float(d) for d in range(0, 2050)] + [d + 0.5 for d in range(0, 40)]
    ds += [2.0**e for e in range(-149, 128, 7)] + [98.0 * 2.0**e for e in range(-30, 100, 9)]
    ds += [float(x) for x in rng.integers(0, 2**32, 300, dtype=np.uint64).astype(np.uint32).view(np.float32)]
    ds += [float(np.float32(x)) for x in (0.03, 0.01, 1e30, 3.4e38, 1e-45, 16777216.0, 16777218.0, 50331648.0)]
    ds += [-d for d in ds] + [float("inf"), float("-inf"), float("nan")]
    args = ["nan" if d != d else float(d).hex() for d in ds]
    out = subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout
    want = "".join("1" if recip_product_exact(d) else "0" for d in ds)
    bad = [ds[i] for i in range(len(ds)) if out[i] != want[i]]
    assert len(out) == len(ds) and not bad, bad[:10]
