"""The C restatements of the variant servers' float32 reductions (oracle/reductions.c).

Pinned two ways, on the CPU:
* against the libraries the reference calls, on this host: numpy's
  ``np.inner`` / ``np.linalg.norm`` (FedAdp) and torch's
  ``F.cosine_similarity`` (Port), over ragged sizes and thread counts;
* against the reference-generated fixtures: Port's similarities and FedAdp's
  adaptive weights, bit for bit.
"""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fedavg_oracle as ref
from oracle import reductions as R
from oracle import synth
from plato_amd import weights as W
from tests import golden_cases as G
from tests import special_values as SV

pytestmark = pytest.mark.skipif(not os.path.exists(R.LIB_PATH), reason="oracle library not built")
CASES = {c["recipe"]["name"]: c for c in G.load_cases()}
SIZES = list(range(1, 70)) + [127, 128, 129, 1000, 32767, 32768, 40001, 65537, 262147]


def _openblas_arch():
    try:
        import threadpoolctl

        for info in threadpoolctl.threadpool_info():
            if info.get("internal_api") == "openblas":
                return info.get("architecture")
    except Exception:  # pragma: no cover
        return None
    return None


SKX_LIKE = ("SkylakeX", "Cooperlake", "SapphireRapids")


@pytest.mark.skipif(_openblas_arch() not in SKX_LIKE, reason="numpy's OpenBLAS picked another CPU kernel here")
def test_sdot_restatement_equals_numpy_inner_and_norm():
    import threadpoolctl

    rng = np.random.default_rng(3)
    for n in SIZES:
        x = rng.standard_normal(n).astype(np.float32)
        y = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        for threads in (1, 4):
            with threadpoolctl.threadpool_limits(threads, user_api="blas"):
                assert R.sdot(x, y) == np.float32(np.inner(x, y)), (n, threads)
                assert R.np_norm(y) == np.linalg.norm(y), (n, threads)


@pytest.mark.parametrize("threads", [1, 2, 3, 8, 16])
def test_torch_reductions_restatement_equals_torch(threads):
    rng = np.random.default_rng(threads)
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        for n in SIZES + [1 << 20, (1 << 20) + 5]:
            a = (rng.standard_normal(n) * 1e-2).astype(np.float32)
            b = (rng.standard_normal(n) * 3e-2).astype(np.float32) + a
            ta, tb = torch.from_numpy(a), torch.from_numpy(b)
            assert R.torch_norm(a) == np.float32(torch.linalg.vector_norm(ta).item()), n
            assert R.torch_sum(b, threads) == np.float32(tb.sum().item()), n
            assert R.torch_cosine(a, b, threads) == np.float32(F.cosine_similarity(ta, tb, dim=0).item()), n
    finally:
        torch.set_num_threads(old)


# ------------------------------------------------------------------ special values
# The restatements against torch and numpy on tests/special_values.py's cases: every value class x
# placement of the special element x size.  Bits are compared; a NaN matches any NaN.  Each test walks
# all sizes and reports every departure at once: (n, placement, got, want).
def _cases(cls, n):
    for p in ([0] if cls in SV.WHOLE else SV.placements(n)):
        yield (p,) + SV.vector_case(cls, n, p)


def _f32(t) -> np.float32:
    return np.float32(t.item())


@pytest.mark.parametrize("cls", SV.CLASSES)
def test_special_values_torch_norm(cls):
    bad = []
    for n in SV.SIZES:
        for p, a, b in _cases(cls, n):
            for v in (a, b):
                got, want = R.torch_norm(v), _f32(torch.linalg.vector_norm(torch.from_numpy(v)))
                if not SV.same_bits(got, want):
                    bad.append((n, p, got, want))
    assert not bad, bad


@pytest.mark.parametrize("shape", [(), (1,), (1, 1)], ids=["0d", "1", "1x1"])
@pytest.mark.parametrize("cls", SV.CLASSES)
def test_special_values_one_element_norm(cls, shape):
    """torch.linalg.norm of any one-element tensor is |x| (FedAtt's scalar entries): 1e-30 and 1e25 come
    back as they are; both restatements follow."""
    bad = []
    for seed in range(4):
        a, b = SV.vector_case(cls, 1, 0, seed)
        for v in (a, b, -a):
            want = _f32(torch.linalg.norm(torch.from_numpy(v).reshape(shape)))
            for got in (R.torch_norm(v), ref.torch_cpu_norm_f32(v[None, :])[0]):
                if not SV.same_bits(got, want):
                    bad.append((v, got, want))
    assert not bad, bad


@pytest.mark.parametrize("x,want", [(1e-30, 1e-30), (-1e-42, 1e-42), (1.049e-20, 1.049e-20), (3e19, 3e19),
                                    (-1e25, 1e25)])
def test_one_element_norm_neither_underflows_nor_overflows(x, want):
    v = np.asarray([x], dtype=np.float32)
    assert R.torch_norm(v).tobytes() == np.float32(want).tobytes()
    assert _f32(torch.linalg.norm(torch.from_numpy(v))).tobytes() == np.float32(want).tobytes()
    assert ref.torch_cpu_norm_f32(v[None, :])[0].tobytes() == np.float32(want).tobytes()


@pytest.mark.parametrize("threads", [1, 4, 16])
@pytest.mark.parametrize("cls", SV.CLASSES)
def test_special_values_torch_cosine_and_sum(cls, threads):
    bad = []
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        for n in SV.SIZES:
            for p, a, b in _cases(cls, n):
                ta, tb = torch.from_numpy(a), torch.from_numpy(b)
                got, want = R.torch_cosine(a, b, threads), _f32(F.cosine_similarity(ta, tb, dim=0))
                if not SV.same_bits(got, want):
                    bad.append(("cosine", n, p, got, want))
                got, want = R.torch_sum(a, threads), _f32(ta.sum())
                if not SV.same_bits(got, want):
                    bad.append(("sum", n, p, got, want))
    finally:
        torch.set_num_threads(old)
    assert not bad, bad


@pytest.mark.skipif(_openblas_arch() not in SKX_LIKE, reason="numpy's OpenBLAS picked another CPU kernel here")
@pytest.mark.parametrize("cls", SV.CLASSES)
def test_special_values_sdot_and_np_norm(cls):
    bad = []
    with np.errstate(all="ignore"):
        for n in SV.SIZES:
            for p, a, b in _cases(cls, n):
                got, want = R.sdot(a, b), np.float32(np.inner(a, b))
                if not SV.same_bits(got, want):
                    bad.append(("inner", n, p, got, want))
                got, want = R.np_norm(a), np.float32(np.linalg.norm(a))
                if not SV.same_bits(got, want):
                    bad.append(("norm", n, p, got, want))
    assert not bad, bad


@pytest.mark.skipif(_openblas_arch() not in SKX_LIKE, reason="numpy's OpenBLAS picked another CPU kernel here")
def test_sdot_of_negative_zero_products():
    """np.inner of one-element vectors is the bare product (-0 stays -0); from n = 2 on the sum starts at +0."""
    for n in list(range(1, 70)) + [127, 128, 129, 1000]:
        x, y = np.full(n, -0.0, np.float32), np.full(n, 1.0, np.float32)
        assert R.sdot(x, y).tobytes() == np.float32(np.inner(x, y)).tobytes(), n
    assert np.signbit(R.sdot(np.float32([-0.0]), np.float32([1.0])))


@pytest.mark.parametrize("cls", SV.CLASSES)
def test_special_values_np_sum_of_squares(cls):
    bad = []
    with np.errstate(all="ignore"):
        for n in SV.SIZES:
            for p, a, b in _cases(cls, n):
                for d in (a, b):
                    got, want = R.np_sum(np.square(d)), np.sum(np.square(d))
                    if not SV.same_bits(got, want):
                        bad.append((n, p, got, want))
    assert not bad, bad


def test_special_value_cases_have_their_class():
    """The builder's own claims, which both halves rest on."""
    with np.errstate(all="ignore"):
        for n in (1, 2, 9, 257, 8193):
            rng = np.random.default_rng(n)
            assert not np.square(SV.whole_values("sub", n, rng)).any()
            sq = np.square(SV.whole_values("tiny", n, rng))
            assert sq.all() and (sq < np.finfo(np.float32).tiny).all()
            big = SV.whole_values("big", n, rng).astype(np.float64)
            assert 0.8 * SV.FLT_MAX < (big * big).sum() < SV.FLT_MAX
            assert np.isinf(R.torch_norm(SV.whole_values("ovf", n + 8, rng)))
            z = SV.whole_values("zeros", n, rng)
            assert not z.any() and np.signbit(z).tolist() == [i % 2 == 1 for i in range(n)]
            for p in SV.placements(n):
                assert R.torch_norm(SV.vector_case("eps_below", n, p)[0]) < SV.EPS
                assert R.torch_norm(SV.vector_case("eps_at", n, p)[0]) == SV.EPS
                assert R.torch_norm(SV.vector_case("eps_above", n, p)[0]) > SV.EPS
                assert np.isnan(SV.vector_case("inf_minus_inf", n, p)[0][p])
    assert SV.placements(8193) == [0, 2047, 2048, 8191, 8192]
    assert SV.placements(13) == [0, 7, 8, 9, 10, 11, 12]
    lay = SV.layout()
    c = SV.arena_case(lay, 3, targets=[(1, "v9", "first", "tiny")])
    rows = SV.entry_rows(c, lay["v9"])
    assert (np.abs(rows[1]) < 2e-19).all() and (np.abs(rows[1]) > 5e-21).all() and (np.abs(rows[0]) > 1e-6).any()
    rows = SV.entry_rows(SV.arena_case(lay, 3), lay["t5"])
    assert rows[0].tolist() == [-2.0**63] * 5 and np.isinf(R.torch_norm(rows[0]))
    groups = SV.spot_groups(lay, 1)
    assert sum(len(g) for g in groups) == len(SV.SPOTS) and len(groups) == 6  # v24579 holds six spots
    assert all(len({(c, n) for c, n, _, _ in g}) == len(g) for g in groups)
    assert {t[3] for r in range(7) for t in SV.spot_groups(lay, 5, r)[0] if t[1] == "s0"} == set(SV.SINGLE)
    c = SV.arena_case(lay, 3, targets=[(2, "v8191", "last", "inf_minus_inf"), (1, "v8192", "first", "nan")])
    assert c["at"] == [lay["v8192"].offset - 1, lay["v8192"].offset]
    assert np.isnan(SV.entry_rows(c, lay["v8191"])[2, -1]) and np.isnan(SV.entry_rows(c, lay["v8192"])[1, 0])
    clean = SV.arena_case(lay, 3)
    p = SV.poisoned(clean, 1, "v9", "ovf")
    assert np.isinf(R.torch_norm(SV.entry_rows(p, lay["v9"])[1]))
    diff = np.argwhere(p["xs_f"].view(np.uint32) != clean["xs_f"].view(np.uint32))
    assert set(diff[:, 0]) == {1} and set(diff[:, 1]) == set(range(lay["v9"].offset, lay["v9"].offset + 9))
    assert (SV.arena_deltas(SV.arena_case(lay, 3))[1][:, lay["t0"].offset] < 0).all()  # they wrap


def _port_vectors(recipe):
    from plato_amd.arena import ArenaLayout

    layout = ArenaLayout.from_shapes(G.model_spec(recipe["model"]))
    k, seed = recipe["k"], recipe["seed"]
    bf, bi = synth.baseline_arena(layout.n_f32, layout.n_i64, seed)
    pv = recipe["previous"]
    pf = synth.synth_f32(layout.n_f32, seed, pv["stream"], pv["scale"], add=bf)
    pi = synth.synth_i64(layout.n_i64, seed, pv["stream"], 3, add=bi)
    v = R.port_current_minus_previous(layout.entries, bf, bi, pf, pi)
    ds = []
    for c in G.order_of(recipe):
        xf, xi = synth.client_arena(bf, bi, seed, c)
        ds.append(R.port_delta(layout.entries, bf, bi, xf, xi))
    return v, ds


# the fixtures were generated with torch's default pool on the 8-CPU survey host
FIXTURE_TORCH_THREADS = 8


@pytest.mark.parametrize("name", ["port_similarity_lenet5_k8", "port_similarity_resnet18_k4"])
def test_port_similarity_restatement_reproduces_reference_bits(name):
    case = CASES[name]
    recipe = case["recipe"]
    v, ds = _port_vectors(recipe)
    sims = G.reference_similarities(case)
    st = [recipe["staleness"][c] for c in G.order_of(recipe)]
    checked = 0
    for i, s in enumerate(sims):
        if st[i] <= 1:
            continue
        got = R.torch_cosine(v, ds[i], FIXTURE_TORCH_THREADS)
        assert got.tobytes() == np.float32(s).tobytes(), (i, got, s)
        checked += 1
    assert checked


LR = 0.01  # parameters.optimizer.lr of the FedAdp fixture config


@pytest.mark.parametrize("name", ["fedadp_lenet5_k6", "fedadp_resnet18_k8"])
def test_fedadp_weights_from_restated_dots_reproduce_reference_bits(name):
    case = CASES[name]
    recipe, exp = case["recipe"], case["expected"]
    layout, base, pays, (bf, bi, xs_f, xs_i) = G.host_state_dicts(recipe)
    ns = [recipe["num_samples"][c] for c in G.order_of(recipe)]
    d_f = [np.subtract(x, bf, dtype=np.float32) for x in xs_f]
    g_f, g_i = ref.deltas_numpy(d_f, [x - bi for x in xs_i], ref.fedavg_weights(ns))
    grads = layout.unpack(torch.from_numpy(g_f), torch.from_numpy(g_i))
    g = ref.fedadp_flatten(grads, LR)
    inner, l_sq = [], []
    for x in pays:
        loc = ref.fedadp_flatten({n: x[n] - base[n] for n in x}, LR)
        inner.append(R.sdot(g, loc))
        l_sq.append(R.sdot(loc, loc))
    angles = W.fedadp_angles_from_dots(inner, R.sdot(g, g), l_sq)
    selected = [c + 1 for c in G.order_of(recipe)]
    local = {int(c): np.float32(float.fromhex(a)) for c, a in recipe.get("local_angles", {}).items()}
    contribs = W.fedadp_contributions(angles, selected, local, recipe["current_round"])
    aw = W.fedadp_weighting(contribs, ns)
    assert [float(x).hex() for x in aw] == exp["adaptive_weighting"]
    assert {str(c): "%08x" % np.float32(a).view(np.uint32) for c, a in local.items()} == exp["local_angles"]


def test_numpy_sum_restatement_equals_np_sum_of_squares():
    rng = np.random.default_rng(11)
    for shape in [(1,), (7,), (8,), (100,), (129,), (8192,), (8193,), (20000,), (100003,), (64, 3, 3, 3),
                  (512, 256, 3, 3)]:
        d = (rng.standard_normal(shape) * 1e-2).astype(np.float32)
        assert R.np_sum(np.square(d).ravel()) == np.sum(np.square(d)), shape


def test_polaris_norms_from_restated_sums_reproduce_reference_bits():
    case = CASES["polaris_resnet18_k8"]
    recipe, exp = case["recipe"], case["expected"]
    layout, base, pays, (bf, bi, xs_f, xs_i) = G.host_state_dicts(recipe)
    names = layout.keys()
    got = {}
    for c, x in zip(G.order_of(recipe), pays):
        sums = np.zeros(len(names), dtype=np.float32)
        for e_i, e in enumerate(layout.entries):
            if e.region == "f32" and "conv" in e.name:
                d = np.subtract(x[e.name].numpy(), base[e.name].numpy(), dtype=np.float32)
                sums[e_i] = R.np_sum(np.square(d).ravel())
        got[c] = W.polaris_delta_norms(sums[None, :], names)[0]
    want = {int(c): float.fromhex(v) for c, v in exp["squared_deltas"].items()}
    assert {c: float(v).hex() for c, v in got.items()} == {c: float(want[c]).hex() for c in got}
    # unexplored clients get alpha * the mean norm, accumulated like the reference (float32 norms)
    total = 0
    for c in got:
        total += got[c]
    expect = 10 * (total / len(got))  # alpha of the fixture config
    assert all(float(want[c]).hex() == float(expect).hex() for c in want if c not in got)
