"""Case generators and host references for the edge-shape tests of the float64, decode, dot-product,
mix / cast and synthetic-fill entry points.

Everything here runs without a device: tests/test_edge_cases.py drives the generators and references on
the CPU and asserts the conditions the GPU comparisons rest on; the GPU modules (tests/test_w64_gpu.py,
tests/test_decode_rows_gpu.py, tests/test_client_dots_gpu.py, tests/test_elementwise_gpu.py) feed the
same cases to the C ABI.  The few device helpers at the end only move host arrays to 16-byte-aligned
device rows with sentinel-filled guards.
"""

from __future__ import annotations

import math
import os
import re

import numpy as np

from oracle import fedavg_oracle as ref
from oracle import qsgd as Q
from plato_amd.arena import ArenaLayout
from tests import golden_cases as G
from tests.test_fuzz_gpu import SPECIAL_F32, SPECIAL_I64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # guard elements behind every output
SENTINEL32 = np.uint32(0xDEADBEEF)  # as fp32 -6.26e18: neither NaN nor a value any case produces
SENTINEL64 = np.uint64(0xDEADBEEFDEADBEEF)  # as fp64 -1.19e148
CANON_NAN64 = np.uint64(0x7FF8000000000000)
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def bits32(a) -> np.ndarray:
    """fp32 values as uint32 after NaN-payload canonicalisation (G.canon)."""
    return G.canon(np.asarray(a, dtype=np.float32)).view(np.uint32)


def bits64(a) -> np.ndarray:
    """fp64 values as uint64 with every NaN written as the canonical quiet NaN."""
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a.view(np.uint64)[np.isnan(a)] = CANON_NAN64
    return a.view(np.uint64)


def _ksu() -> int:
    """kSU of fedavg_agg.hip: the scalar items' client-load batch, an unroll edge of plato_agg_fedavg_w64."""
    text = open(os.path.join(ROOT, "plato_amd", "csrc", "fedavg_agg.hip")).read()
    return int(re.search(r"constexpr int kSU = (\d+);", text).group(1))


# ------------------------------------------------------------------------------------------------
# 1. plato_agg_fedavg_w64
# ------------------------------------------------------------------------------------------------
K_SU = _ksu()
W64_KS = tuple(sorted({1, 2, 3, 4, 5, 7, 8, 9, 16, 17, K_SU - 1, K_SU, K_SU + 1}))
W64_NF = (0, 1, 3, 4, 5, 255, 1023, 1024, 1025, 1027, 70_001)
W64_NI = (0, 1, 7, 300)  # 300 + a 3-element fp32 tail: more than 256 scalar items, two scalar workgroups
W64_SHAPES = tuple((nf, ni) for nf in W64_NF for ni in W64_NI if nf + ni > 0)
# float64 weights the fp32 cast would change or lose: not fp32-representable, signed zeros, subnormal
# doubles, and +-1e300 whose products overflow fp32 to +-inf in the accumulator's cast
HARD_W64 = (0.0, -0.0, 5e-324, 1e-310, 1e300, -1e300, 1.0 / 3.0, 0.1, -2.0 / 7.0)


def w64_seed(k: int, shape_index: int) -> int:
    return W64_KS.index(k) * len(W64_SHAPES) + shape_index


def w64_is_special(seed: int) -> bool:
    return seed % 3 == 0


def w64_case(k: int, n_f: int, n_i: int, seed: int) -> dict:
    """Values as tests/test_fuzz_gpu.py draws them (every third seed: 2 % special fp32 values, 20 % special
    int64 values whose differences wrap), float64 weights of four kinds, a separate fp32 weight vector for
    the int64 entries, the clients in a permuted order."""
    rng = np.random.default_rng(20_000 + seed)
    special = w64_is_special(seed)
    base_f = (rng.standard_normal(n_f) * 0.05).astype(np.float32)
    xs_f = (base_f[None, :] + rng.standard_normal((k, n_f)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    base_i = rng.integers(0, 10_000, n_i, dtype=np.int64)
    xs_i = base_i[None, :] + rng.integers(0, 9, (k, n_i), dtype=np.int64)
    if special:
        for arr in (base_f, xs_f.reshape(-1)):
            if arr.size:
                m = rng.random(arr.size) < 0.02
                arr[m] = rng.choice(SPECIAL_F32, int(m.sum()))
        for arr in (base_i, xs_i.reshape(-1)):
            if arr.size:
                m = rng.random(arr.size) < 0.2
                arr[m] = rng.choice(SPECIAL_I64, int(m.sum()))
    kind = seed % 4
    if kind == 0:  # n_i / N
        ns = rng.integers(100, 2000, k)
        w64 = [float(n) / float(ns.sum()) for n in ns]
    elif kind == 1:  # doubles that are not fp32-representable
        w64 = [float(a * b) for a, b in zip(rng.choice([1.0 / 3.0, 0.1, -2.0 / 7.0, 1.0 / 7.0], k),
                                            rng.uniform(0.5, 2.0, k))]
    elif kind == 2:
        w64 = [float(x) for x in rng.choice(HARD_W64, k)]
    else:  # any sign and magnitude; one NaN weight (not in the special seeds, whose NaN share is bounded)
        w64 = [float(x) for x in rng.standard_normal(k) * 10.0 ** rng.integers(-3, 3, k)]
        if not special:
            w64[int(rng.integers(k))] = float("nan")
    if seed % 5 == 2:
        w_i64 = [float(x) for x in rng.choice([0.0, -0.0, 1e-42, 0.5, -2.0, 1.0 / 3.0, 1e30], k)]
    else:
        w_i64 = [float(x) for x in rng.standard_normal(k)]
    return dict(k=k, n_f=n_f, n_i=n_i, seed=seed, special=special, base_f=base_f, xs_f=xs_f, base_i=base_i,
                xs_i=xs_i, w64=w64, w_i64=w_i64, order=[int(j) for j in rng.permutation(k)])


def w64_reference(c: dict, has_base: bool):
    """oracle.fedavg_oracle.w64_numpy on the case, clients and weights in the case's order."""
    o = c["order"]
    with np.errstate(all="ignore"):
        return ref.w64_numpy([c["xs_f"][j] for j in o], [c["xs_i"][j] for j in o], [c["w64"][j] for j in o],
                             [c["w_i64"][j] for j in o], c["base_f"] if has_base else None,
                             c["base_i"] if has_base else None)


def w64_composed(c: dict):
    """What the base mode claims to be: update(b, w64_numpy(x - b)), the subtraction in fp32, the int64
    difference wrapping (compute_weight_deltas), b + avg in fp32 (update_weights)."""
    o = c["order"]
    with np.errstate(all="ignore"):
        d_f = [np.subtract(c["xs_f"][j], c["base_f"], dtype=np.float32) for j in o]
        d_i = [(c["xs_i"][j].view(np.uint64) - c["base_i"].view(np.uint64)).view(np.int64) for j in o]
        avg_f, avg_i = ref.w64_numpy(d_f, d_i, [c["w64"][j] for j in o], [c["w_i64"][j] for j in o])
        return (np.add(c["base_f"], avg_f, dtype=np.float32),
                np.add(c["base_i"].astype(np.float32), avg_i, dtype=np.float32))


def nan_share(*arrays) -> float:
    n = sum(a.size for a in arrays)
    return sum(int(np.isnan(a).sum()) for a in arrays) / n if n else 0.0


# ------------------------------------------------------------------------------------------------
# 2. plato_agg_weighted_sum_f64
# ------------------------------------------------------------------------------------------------
F64_NS = (1, 2, 3, 255, 256, 257, 511, 513, 100_003)
F64_KS = (1, 2, 3, 4, 5, 8, 9)
SPECIAL_F64 = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e308, -1e308, np.inf, -np.inf, np.nan])
SPECIAL_W64 = np.array([0.0, -0.0, 5e-324, 1e-310, 1e308, -1e308, 1.0 / 3.0])


def f64_case(k: int, n: int, seed: int):
    rng = np.random.default_rng(30_000 + seed)
    xs = rng.standard_normal((k, n))
    m = rng.random(xs.shape) < (0.5 if n <= 3 else 0.05)
    xs[m] = rng.choice(SPECIAL_F64, int(m.sum()))
    w = rng.standard_normal(k)
    m = rng.random(k) < 0.3
    w[m] = rng.choice(SPECIAL_W64, int(m.sum()))
    if seed % 4 == 3:
        w[int(rng.integers(k))] = rng.choice([np.inf, -np.inf, np.nan])
    return xs, w


def f64_reference(xs: np.ndarray, w) -> np.ndarray:
    """acc = acc + x_i * w_i in numpy float64 from +0.0, clients in order (fedavg_he.py:88-98)."""
    acc = np.zeros(xs.shape[1], dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(xs.shape[0]):
            acc = acc + np.asarray(xs[i], dtype=np.float64) * np.float64(w[i])
    return acc


# ------------------------------------------------------------------------------------------------
# 3. plato_agg_decode_rows
# ------------------------------------------------------------------------------------------------
DECODE_CAPS = (4, 256, 4096)
DECODE_KS = (1, 2, 5)
QSGD_MAX_V = np.array([0.0, 1e-45, 1.17e-38, 1e-3, 1.0, 3.4e38, np.inf, np.nan], dtype=np.float32)
# 98 and 246: even, no power of two, where an exact tie between two subnormals exists (tests/test_division.py)
QSGD_DIVISORS = (1, 3, 127, 255, 98, 246)
NATIVE_I64 = np.array([0, 1, -1, 2**24 + 1, -(2**24 + 1), 2**24 + 3, -(2**24 + 3), 2**53 + 1, I64_MIN, I64_MAX],
                      dtype=np.int64)  # 2^24 + 1 and 2^24 + 3 are ties: RNE gives 2^24 and 2^24 + 4


def decode_layout(with_i64: bool) -> ArenaLayout:
    """Entries of 0, 1, 5, 255, 256, 257 and 5000 elements (chunk pieces shorter than, equal to and longer
    than the kernel's 256-lane stride), int64 scalars first, between and last, one int64 entry of 3
    elements; eight 256-element entries per region (QSGD: every code byte under every max_v) and one entry
    of >= 65536 elements per region (bf16: every bit pattern).  Without an int64 region the fp32 entries
    are FedAdp-aligned, so the fp32 region itself has padding between entries that must stay untouched."""
    spec = []

    def i64(name, shape):
        if with_i64:
            spec.append((name, shape, "i64"))

    i64("c_first", ())
    for n in (0, 1, 5):
        spec.append((f"e{n}", (n,), "f32"))
    i64("c3", (3,))
    for n in (255, 256, 257, 5000):
        spec.append((f"e{n}", (n,), "f32"))
        if n == 256:
            i64("c_mid", ())
    for j in range(8):
        spec.append((f"q{j}", (16, 16), "f32"))
        i64(f"qc{j}", (256,))
    spec.append(("big", (256, 257), "f32"))  # the QSGD wire header holds each dimension as an int16
    i64("cbig", (256, 256))
    i64("c_last", ())
    return ArenaLayout.from_shapes(spec, align=None if with_i64 else "fedadp")


def decode_sources(layout: ArenaLayout, codec: str, k: int, seed: int):
    """Per client the two source arenas in the codec's element type, and max_v [n_entries][K] (QSGD)."""
    rng = np.random.default_rng(40_000 + seed)
    n_f, n_i, n_e = layout.n_f32, layout.n_i64, len(layout.entries)
    src_f, src_i, mv = [], [], None
    if codec == "bf16":  # every one of the 65,536 patterns in each region of each client
        perm = rng.permutation(1 << 16).astype(np.uint16)
        for c in range(k):
            src_f.append(perm[(np.arange(n_f) + 7919 * c) % (1 << 16)])
            src_i.append(perm[(np.arange(n_i) + 104_729 * c + 17) % (1 << 16)])
    elif codec == "qsgd":
        # distinct ordinary values everywhere (a transposed or wrong-stride index reads another one), the
        # hostile pool on the 256-element entries, rotated so that every (byte, max_v) pair occurs
        mv = rng.uniform(0.01, 3.0, (n_e, k)).astype(np.float32)
        q_entries = [e_i for e_i, e in enumerate(layout.entries) if e.numel == 256 and e.name.startswith("q")]
        for j, e_i in enumerate(q_entries):
            for c in range(k):
                mv[e_i, c] = QSGD_MAX_V[(j + 3 * c + seed) % len(QSGD_MAX_V)]
        for c in range(k):
            cf = rng.integers(0, 256, n_f).astype(np.uint8)
            ci = rng.integers(0, 256, n_i).astype(np.uint8)
            for e_i in q_entries:
                e = layout.entries[e_i]
                (cf if e.region == "f32" else ci)[e.offset:e.offset + 256] = rng.permutation(256).astype(np.uint8)
            src_f.append(cf)
            src_i.append(ci)
    else:  # native: any fp32 bit pattern (NaN payloads included); int64 extremes and RNE ties
        for c in range(k):
            src_f.append(rng.integers(0, 1 << 32, n_f, dtype=np.uint64).astype(np.uint32).view(np.float32))
            xi = rng.integers(-(1 << 62), 1 << 62, n_i, dtype=np.int64)
            small = rng.random(n_i) < 0.5
            xi[small] = rng.integers(-(1 << 26), 1 << 26, int(small.sum()), dtype=np.int64)
            if n_i:
                big = layout["cbig"]
                xi[big.offset:big.offset + NATIVE_I64.size] = np.roll(NATIVE_I64, c)
                xi[layout["c3"].offset:layout["c3"].offset + 3] = np.roll(NATIVE_I64, c)[3:6]
                xi[layout["c_first"].offset] = NATIVE_I64[(8 + c) % NATIVE_I64.size]
                xi[layout["c_mid"].offset] = NATIVE_I64[(7 + c) % NATIVE_I64.size]
                xi[layout["c_last"].offset] = NATIVE_I64[(9 + c) % NATIVE_I64.size]
            src_i.append(xi)
    return src_f, src_i, mv


def qsgd_chain(codes: np.ndarray, max_v, divisor) -> np.ndarray:
    """fp32(fp32(fp32(zeta) * max_v) / divisor), zeta = -(byte - 128) for byte >= 128 else byte."""
    raw = codes.astype(np.int64)
    zeta = np.where(raw >= 128, -(raw - 128), raw).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.divide(np.multiply(zeta, np.float32(max_v), dtype=np.float32), np.float32(divisor),
                         dtype=np.float32)


def decode_values(layout: ArenaLayout, codec: str, src_f, src_i, mv_client, divisor):
    """One client's decoded regions as uint32 bit patterns (QSGD: NaN payloads canonicalised)."""
    if codec == "native":
        return src_f.view(np.uint32), src_i.astype(np.float32).view(np.uint32)  # numpy's int64 -> fp32: RNE
    if codec == "bf16":
        return src_f.astype(np.uint32) << 16, src_i.astype(np.uint32) << 16  # exact widening
    with np.errstate(all="ignore"):
        vf, vi = Q.dequantize_regions(layout.entries, src_f, src_i, mv_client, level=int(divisor) + 1)
    return bits32(vf), bits32(vi)


def decode_expected_row(layout: ArenaLayout, vf: np.ndarray, vi: np.ndarray, dst_off: int, row_len: int):
    """The destination row after the call: the sentinel everywhere but at the entries' elements."""
    row = np.full(row_len, SENTINEL32, dtype=np.uint32)
    for e in layout.entries:
        src, at = (vf, e.offset) if e.region == "f32" else (vi, dst_off + e.offset)
        row[at:at + e.numel] = src[e.offset:e.offset + e.numel]
    return row


# ------------------------------------------------------------------------------------------------
# 4. plato_agg_client_dots
# ------------------------------------------------------------------------------------------------
DOTS_KS = (1, 7, 8, 9, 17)  # the edges of kU = 8
DOTS_NF = (0, 1, 3, 4, 5, 1023, 1024, 1025, 1027, 4099, 300_003)  # the last: more than 256 chunk partials
DOTS_NI = (0, 1, 5)


def dots_case(kind: str, k: int, n_f: int, n_i: int, has_base: bool, seed: int, wrap: bool = False) -> dict:
    rng = np.random.default_rng(50_000 + seed)
    if kind == "exact":  # small integers: every product and partial sum is an exact double
        b = rng.integers(-64, 65, n_f).astype(np.float32)
        x = rng.integers(-64, 65, (k, n_f)).astype(np.float32)
        v = rng.integers(-64, 65, n_f).astype(np.float32)
        bi = rng.integers(-1000, 1000, n_i, dtype=np.int64)
        xi = bi[None, :] + rng.integers(-500, 500, (k, n_i), dtype=np.int64)
        vi = rng.integers(-1000, 1000, n_i, dtype=np.int64)
    else:
        b = rng.standard_normal(n_f).astype(np.float32)
        x = rng.standard_normal((k, n_f)).astype(np.float32)
        v = rng.standard_normal(n_f).astype(np.float32)
        bi = rng.integers(-10**6, 10**6, n_i, dtype=np.int64)
        xi = bi[None, :] + rng.integers(-50, 50, (k, n_i), dtype=np.int64)
        vi = rng.integers(-1000, 1000, n_i, dtype=np.int64)
        if wrap:  # int64 differences that wrap (needs a base and n_i64 >= 2)
            bi[0], bi[1] = -2, I64_MIN
            xi[:, 0] = I64_MAX - np.arange(k)
            xi[:, 1] = 5 + np.arange(k)
    return dict(kind=kind, k=k, n_f=n_f, n_i=n_i, has_base=has_base, b=b, x=x, v=v, bi=bi, xi=xi, vi=vi)


def dots_vectors(c: dict):
    """(d [K, n], v [n]) in fp32 as the kernel forms them: d = x - b in fp32 as compute_weight_deltas does
    (or x), int64 entries fp32(int64 x - b) with the difference wrapping (or fp32(x)); v's int64 as fp32."""
    if c["has_base"]:
        d_f = np.subtract(c["x"], c["b"][None, :], dtype=np.float32)
        d_i = (c["xi"].view(np.uint64) - c["bi"].view(np.uint64)[None, :]).view(np.int64).astype(np.float32)
    else:
        d_f, d_i = c["x"], c["xi"].astype(np.float32)
    return np.concatenate([d_f, d_i], axis=1), np.concatenate([c["v"], c["vi"].astype(np.float32)])


def dots_reference_exact(c: dict):
    """The 2K+1 outputs as integers, and the largest sum of |terms| of any output: below 2^53 every partial
    sum, in whatever order, is an exact double, so the kernel must return exactly these integers."""
    d, v = dots_vectors(c)
    di, vi = d.astype(np.int64), v.astype(np.int64)
    assert np.array_equal(di.astype(np.float32), d) and np.array_equal(vi.astype(np.float32), v)
    out = [int((di[i] * vi).sum()) for i in range(c["k"])] + [int((di[i] * di[i]).sum()) for i in range(c["k"])]
    out.append(int((vi * vi).sum()))
    abs_sums = [int(np.abs(di[i] * vi).sum()) for i in range(c["k"])] + out[c["k"]:]
    return out, max(abs_sums)


def dots_reference_general(c: dict):
    """(reference [2K+1], bound [2K+1]): math.fsum over the exact double products, and the allowed error.

    The kernel adds the n = n_f32 + n_i64 exact products t_i in some fixed order with one fp64 rounding
    per addition.  Each of the at most n - 1 additions an element passes through multiplies its
    contribution by (1 + delta), |delta| <= 2^-53, so any order errs by at most
    ((1 + 2^-53)^(n-1) - 1) * sum|t_i| = (n - 1) * 2^-53 * sum|t_i| to first order.  The bound allowed is
    n * 2^-52 * fsum(|t_i|): twice the first-order term, which covers the higher-order terms (n * 2^-53 is
    below 1e-10 here) and fsum's own final rounding (2^-53 * |sum|)."""
    d, v = dots_vectors(c)
    d64, v64 = d.astype(np.float64), v.astype(np.float64)
    n, k = v.size, c["k"]
    ref_out, bound = [], []

    def put(t, positive=False):
        ref_out.append(math.fsum(t.tolist()))
        bound.append(n * 2.0**-52 * (ref_out[-1] if positive else math.fsum(np.abs(t).tolist())))

    for i in range(k):
        put(d64[i] * v64)  # exact: 24-bit x 24-bit significands
    for i in range(k):
        put(d64[i] * d64[i], positive=True)
    put(v64 * v64, positive=True)
    return np.asarray(ref_out), np.asarray(bound)


# ------------------------------------------------------------------------------------------------
# 5. cast
# ------------------------------------------------------------------------------------------------
def cast_values() -> np.ndarray:
    """4096 seeded floats of every magnitude, every power of two from 2^-149 to 2^127 with both signs, and
    the fp32 neighbours of +-2^63."""
    rng = np.random.default_rng(60_000)
    vals = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-3, 22, 4096)).astype(np.float32)
    pows = np.ldexp(np.float32(1.0), np.arange(-149, 128)).astype(np.float32)
    edge = np.float32(2.0**63)
    near = np.array([np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(np.inf))],
                    dtype=np.float32)
    return np.concatenate([vals, pows, -pows, near, -near]).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# device helpers (GPU modules only)
# ------------------------------------------------------------------------------------------------
def device_rows(mat: np.ndarray, dev):
    """The rows of a host matrix [K, n] as K device rows, each 16-byte aligned (and, where n allows, no
    better than that); the padding holds 0xFF bytes.  Returns (the tensor that owns them, the K pointers)."""
    import torch

    mat = np.ascontiguousarray(mat)
    k, n = mat.shape
    item = mat.dtype.itemsize
    row = max(16, -(-n * item // 16) * 16)
    host = np.full((k, row), 0xFF, dtype=np.uint8)
    host[:, :n * item] = mat.view(np.uint8).reshape(k, n * item)
    t = torch.from_numpy(host).to(dev)
    return t, [t.data_ptr() + r * row for r in range(k)]


def device_array(a: np.ndarray, dev):
    """A host array on the device (as raw bytes; at least 16 bytes so that the pointer is never null)."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if raw.size < 16:
        raw = np.concatenate([raw, np.zeros(16 - raw.size, np.uint8)])
    return torch.from_numpy(raw.copy()).to(dev)


def pointer_table(ptrs, dev):
    import torch

    return torch.tensor([int(p) for p in ptrs], dtype=torch.int64, device=dev)


def guarded(n: int, sentinel, dev):
    """n + GUARD elements of the sentinel's width, every one holding the sentinel."""
    import torch

    return torch.from_numpy(np.full(n + GUARD, sentinel).view(np.uint8)).to(dev)


def fetch(t, dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


def device_dots(c: dict, dev) -> np.ndarray:
    """The 2K+1 doubles of plato_agg_client_dots on a case of dots_case: two calls that must agree bitwise,
    sentinel-filled outputs and workspace with guards behind them."""
    import torch

    from plato_amd import _lib

    k, n_f, n_i, has_base = c["k"], c["n_f"], c["n_i"], c["has_base"]
    keep_f, pf = device_rows(c["x"], dev)
    keep_i, pi = device_rows(c["xi"], dev)
    tf, ti = pointer_table(pf, dev), pointer_table(pi, dev)
    b, bi = device_array(c["b"], dev), device_array(c["bi"], dev)
    v, vi = device_array(c["v"], dev), device_array(c["vi"], dev)
    ws_bytes = _lib.lib().plato_agg_client_dots_workspace(k, n_f)
    assert ws_bytes % 8 == 0 and ws_bytes >= (2 * k + 1) * 8
    outs = []
    for _ in range(2):
        ws = guarded(ws_bytes // 8, SENTINEL64, dev)
        out = guarded(2 * k + 1, SENTINEL64, dev)
        _lib.call("plato_agg_client_dots", tf.data_ptr(), ti.data_ptr() if n_i else None, k,
                  b.data_ptr() if has_base else None, bi.data_ptr() if has_base and n_i else None, v.data_ptr(),
                  vi.data_ptr() if n_i else None, n_f, n_i, ws.data_ptr(), out.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        got, got_ws = fetch(out, np.uint64), fetch(ws, np.uint64)
        assert (got[2 * k + 1:] == SENTINEL64).all(), "guard doubles behind d_out overwritten"
        assert (got_ws[ws_bytes // 8:] == SENTINEL64).all(), "guard doubles behind the workspace overwritten"
        assert not (got[:2 * k + 1] == SENTINEL64).any(), "an output was not written"
        outs.append(got[:2 * k + 1].copy())
    assert outs[0].tobytes() == outs[1].tobytes(), "two calls on the same inputs differ"
    return outs[0].view(np.float64)
