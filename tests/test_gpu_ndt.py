"""GPU tests of the Normal Distributions Transform (rules N1-N12 in include/mvr_hip.h) against the numpy reference
tests/ndt_ref.py on the cases of tests/ndt_cases.py: the cells, the 29 sums, the two lookups, the whole align with its trace,
its exits and its output slot."""
import importlib

import numpy as np
import pytest

import ndt_cases as NC
import ndt_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17
SUM_TOL = 1e-10                          # tests/test_gpu_gicp.py: of the sum of the terms' absolute values
S, T_, O = 0, 1, 2


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    with mvr.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def ref_cells():
    cache = {}

    def get(case):
        if case["name"] not in cache:
            cache[case["name"]] = R.build_cells(case["tgt"], R.params(**case["prm"]))
        return cache[case["name"]]
    return get


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def load(ctx, case):
    ctx.upload(S, case["src"])
    ctx.upload(T_, case["tgt"])


CELL_CASES = [lambda: NC.centred("res5"), lambda: NC.centred("res10"), lambda: NC.far("res5"), NC.lattice, NC.voxel_edges, NC.nonfinite,
              NC.lane_edges, NC.weight_guard, NC.sparse_native]


@pytest.mark.parametrize("make", CELL_CASES, ids=["centred-res5", "centred-res10", "far-res5", "lattice", "voxel_edges", "nonfinite", "lane_edges",
                                                  "weight_guard", "sparse_native"])
def test_cells(mvr, ctx, ref_cells, make):
    """keys and counts exact; means within 1e-12 (|m| + resolution); C^-1 within 1e-9 of its largest entry (the eigenvalue ratio
    is capped at 100, so two eigen-solvers in f64 agree to about 1e-13: the observed figure is printed)"""
    case = make()
    exp, res = ref_cells(case), case["prm"]["resolution"]
    load(ctx, case)
    got = ctx.ndt_cells(T_, mvr.ndt_params(**case["prm"]))
    assert np.array_equal(got["key"], exp["key"]) and np.array_equal(got["count"], exp["count"]) and len(exp["key"]) > 0
    em = np.abs(got["mean"] - exp["mean"]) / (np.abs(exp["mean"]) + res)
    ec = np.abs(got["icov"] - exp["icov"]).max(1) / np.abs(exp["icov"]).max(1)
    print("%s: %d cells, largest eigenvalue ratio %.3g, %d inflated; means within %.3g, C^-1 within %.3g"
          % (case["name"], len(exp["key"]), exp["eig_ratio"].max(), exp["inflated"].sum(), em.max(), ec.max()))
    assert em.max() <= 1e-12 and ec.max() <= 1e-9 and exp["eig_ratio"].max() <= 100.0 * (1 + 1e-12)
    if case["name"] == "lattice":
        assert np.array_equal(got["mean"], exp["mean"]) and np.abs(got["icov"] - np.array([8 / 7, 0, 0, 8 / 7, 0, 8 / 7])).max() <= 4e-16
    if case["name"] == "voxel_edges":
        # 6, 7, 5 000 and the planar 40; the voxel of 5 and the coincident 9 are no cells
        assert sorted(got["count"]) == [6, 7, 40, 5000] and exp["inflated"].sum() >= 1


def test_cells_at_the_edges_of_the_cell_kernel(mvr, ctx, ref_cells):
    """many_voxels: the voxel loop laps (more voxels than the 64 n_cu waves), every voxel is a cell, n / 3 of them -- one below
    the capacity -- and all planar; a target of three points is one cell, one of two is none.  lane_edges: voxels of 63 ... 129
    points, two collinear ones against their closed form, one with a covariance of 1e-9.  sparse_native: `centred`'s cells, bit
    for bit, from a lattice of more than 1 << 24 voxels."""
    n_cu = int(ctx.stat("n_cu"))
    case = NC.many_voxels(n_cu)
    exp, p = ref_cells(case), mvr.ndt_params(**case["prm"])
    load(ctx, case)
    got = ctx.ndt_cells(T_, p)
    n = len(case["tgt"])
    assert case["n_voxels"] > 64 * n_cu and len(got["key"]) == n // 3 == case["n_voxels"] == n // 3 + 1 - 1 and exp["lat"][2][2] == 1
    assert np.array_equal(got["key"], exp["key"]) and (got["count"] == 3).all() and exp["inflated"].all()
    em = np.abs(got["mean"] - exp["mean"]) / (np.abs(exp["mean"]) + 4.0)
    ec = np.abs(got["icov"] - exp["icov"]).max(1) / np.abs(exp["icov"]).max(1)
    print("many_voxels: %d cells over %d waves; means within %.3g, C^-1 within %.3g" % (len(got["key"]), 64 * n_cu, em.max(), ec.max()))
    assert em.max() <= 1e-12 and ec.max() <= 1e-9
    three = NC.cloud([[1.0, 1.0, 1.0], [3.0, 1.25, 1.0], [1.5, 3.0, 1.0]])
    ctx.upload(T_, three)
    one, want = ctx.ndt_cells(T_, p), R.build_cells(three, R.params(**case["prm"]))
    assert list(one["count"]) == [3] and list(one["key"]) == [0] and np.abs(one["mean"] - want["mean"]).max() <= 1e-12
    assert np.abs(one["icov"] - want["icov"]).max() <= 1e-9 * np.abs(want["icov"]).max()
    ctx.upload(T_, three[:2])
    assert len(ctx.ndt_cells(T_, p)["key"]) == 0
    ctx.upload(S, three)
    assert ctx.ndt_align(S, T_, -1, p)[3] == mvr.E_NOCORR

    case = NC.lane_edges()
    load(ctx, case)
    got = ctx.ndt_cells(T_, mvr.ndt_params(**case["prm"]))
    assert sorted(got["count"]) == sorted(case["counts"]) and ref_cells(case)["inflated"].sum() == 2
    t = case["tgt"][:, :3].astype(np.float64)
    for key, rows in ((case["diagonal_key"], slice(576, 586)), (case["axis_key"], slice(586, 596))):
        k = list(got["key"]).index(key)
        want = NC.line_icov(t[rows])
        assert got["count"][k] == 10 and np.abs(got["icov"][k] - want).max() <= 1e-9 * np.abs(want).max(), (key, got["icov"][k], want)
    tiny = list(got["count"]).index(6)
    assert 1e8 < np.abs(got["icov"][tiny]).max() < 1e11                 # a covariance of (1e-4)^2: kept, and inverted

    base, case = NC.centred("res5"), NC.sparse_native()
    div = ref_cells(case)["lat"][2]
    assert int(div[0]) * int(div[1]) * int(div[2]) > 1 << 24
    load(ctx, base)
    want = ctx.ndt_cells(T_, mvr.ndt_params(**base["prm"]))
    load(ctx, case)
    got = ctx.ndt_cells(T_, mvr.ndt_params(**case["prm"]))
    assert np.array_equal(got["count"], want["count"]) and all(np.array_equal(bits(got[k]), bits(want[k])) for k in ("mean", "icov"))
    sums = [ctx.ndt_sums(S, T_, mvr.ndt_params(**case["prm"]), pose) for pose in NC.poses()]
    load(ctx, base)
    for pose, mine in zip(NC.poses(), sums):
        assert np.array_equal(bits(mine), bits(ctx.ndt_sums(S, T_, mvr.ndt_params(**base["prm"]), pose)))


def sum_cases(n_cu):
    cases = [NC.centred("res5"), NC.centred("res10"), NC.far("res5"), NC.guess("res5"), NC.lattice(), NC.voxel_edges(), NC.nonfinite(), NC.disjoint()]
    cases += [NC.ragged(n) for n in (1, 65, 255, 256, 257, 256 * n_cu + 1)]
    cases += [NC.many_voxels(n_cu), NC.lane_edges(), NC.borders(), NC.weight_guard(), NC.sparse_native()]
    return cases


def check_sums(got, exp, mag, what):
    assert got[27] == exp[27], (what, got[27], exp[27])
    err = np.abs(got - exp)
    assert (err <= SUM_TOL * mag).all(), (what, err / np.maximum(mag, 1e-300))
    return float(np.max(err[mag > 0] / mag[mag > 0])) if (mag > 0).any() else 0.0


def test_sums(mvr, ctx, ref_cells):
    """the count exact, every other sum within SUM_TOL of the sum of its terms' absolute values -- at identity, p* / 2 and p*, on
    every case (the sources of 1 ... 257 points and the one that laps the grid-stride loop included), through the dense table
    and through the search of the kept keys, twice: the four results are the same bits"""
    n_cu = int(ctx.stat("n_cu"))
    assert n_cu > 0
    worst = 0.0
    for case in sum_cases(n_cu):
        prm, p = R.params(**case["prm"]), mvr.ndt_params(**case["prm"])
        cells = ref_cells(case)
        load(ctx, case)
        for pose in NC.poses() + ([case["beyond"]] if "beyond" in case else []):
            exp, mag = R.sums(case["src"], cells, prm, pose, case["G"], with_abs=True)
            got = ctx.ndt_sums(S, T_, p, pose, case["G"])
            ratio = check_sums(got, exp, mag, case["name"])
            worst = max(worst, ratio)
            ctx.tune(ndt_dense_max=0)
            sparse = [ctx.ndt_sums(S, T_, p, pose, case["G"]) for _ in range(2)]
            ctx.tune(ndt_dense_max=1 << 24)
            again = ctx.ndt_sums(S, T_, p, pose, case["G"])
            assert all(np.array_equal(bits(got), bits(o)) for o in sparse + [again]), case["name"]
            print("%s, %d points, |p| %.3g: %d pairs, worst |sum - reference| / sum |terms| = %.3g"
                  % (case["name"], len(case["src"]), np.abs(pose).max(), got[27], ratio))
        if case["name"] == "disjoint":
            assert got[27] == 0 and not got.any()
        if case["name"] == "lattice":
            assert ctx.ndt_sums(S, T_, p)[27] == 13 and ctx.ndt_sums(S, T_, p, case["beyond"])[27] == 12
        if case["name"] == "borders":
            check_borders(mvr, ctx, case)
    assert worst < SUM_TOL


def check_borders(mvr, ctx, case):
    """rule N5 at the rim of the lattice, point by point and through both lookups: a home voxel one outside (h = -1, h = div)
    still sees the rim -- one pair at squared distance 9 --, two outside sees nothing, and so do the two huge finite points"""
    p = mvr.ndt_params(**case["prm"])
    d1, d2, _ = R.constants(4.0, 0.55)
    term = -d1 * np.exp(-d2 * (8 / 7) * 9.0 / 2)
    for dense_max in (1 << 24, 0):
        ctx.tune(ndt_dense_max=dense_max)
        for k, pt in enumerate(case["src"]):
            ctx.upload(S, pt[None])
            got = ctx.ndt_sums(S, T_, p)
            if k < case["n_counted"]:
                assert got[27] == 1 and abs(got[28] - term) <= 1e-13 * term, (k, pt, got[27:])
            else:
                assert not got.any(), (k, pt, got)
    ctx.tune(ndt_dense_max=1 << 24)
    ctx.upload(S, case["src"])
    whole = ctx.ndt_sums(S, T_, p)
    assert whole[27] == case["n_counted"] == len(case["pairs"]) and abs(whole[28] - case["n_counted"] * term) <= 1e-13 * whole[28]


def test_weight_guard_skips_a_pair_whole(mvr, ctx, ref_cells):
    """d2 > 1 at resolution 0.002, outlier ratio 0.99: a pair with q < 2 ln(d2) / d2 has w > 1 and rule N6 skips it -- not
    counted, nothing added to any of the 29 sums.  Point by point, through both lookups."""
    case = NC.weight_guard()
    prm, p = R.params(**case["prm"]), mvr.ndt_params(**case["prm"])
    cells = ref_cells(case)
    assert len(cells["key"]) == 1 and mvr.ndt_constants(p)[1] > 1.0
    ctx.upload(T_, case["tgt"])
    for dense_max in (0, 1 << 24):
        ctx.tune(ndt_dense_max=dense_max)
        for k, want in enumerate(NC.GUARD_COUNTS):
            ctx.upload(S, case["src"][k:k + 1])
            got = ctx.ndt_sums(S, T_, p)
            exp, mag = R.sums(case["src"][k:k + 1], cells, prm, with_abs=True)
            assert got[27] == exp[27] == want and (np.abs(got - exp) <= SUM_TOL * mag).all(), (k, got, exp)
            assert got.any() == bool(want)
    ctx.upload(S, case["src"])
    assert ctx.ndt_sums(S, T_, p)[27] == sum(NC.GUARD_COUNTS)


def test_sums_at_large_angles(mvr, ctx, ref_cells):
    """the D and DD matrices of the pose at angles of radians and 1e-3 from ry = pi / 2 (the reference's are held to central
    differences in tests/test_ndt_host.py): the count exact, the sums within SUM_TOL of the sums of their terms' magnitudes"""
    for case, pose in NC.big_angles():
        prm, p = R.params(**case["prm"]), mvr.ndt_params(**case["prm"])
        load(ctx, case)
        exp, mag = R.sums(case["src"], ref_cells(NC.centred("res5")), prm, pose, case["G"], with_abs=True)
        got = ctx.ndt_sums(S, T_, p, pose, case["G"])
        ratio = check_sums(got, exp, mag, case["name"])
        print("%s: %d pairs, worst |sum - reference| / sum |terms| = %.3g" % (case["name"], got[27], ratio))
        assert got[27] > 1900 and ratio < SUM_TOL


def test_nonfinite_points_count_for_nothing(mvr, ctx):
    """the sums with a NaN source point and a NaN and an infinite target point are the sums without those points (the same
    cells; the source's other points keep their places in the reduction only up to the removed one, so: to SUM_TOL)"""
    case = NC.nonfinite()
    clean, p = case["clean"], mvr.ndt_params(**case["prm"])
    load(ctx, case)
    dirty_cells, dirty = ctx.ndt_cells(T_, p), [ctx.ndt_sums(S, T_, p, pose) for pose in NC.poses()]
    load(ctx, clean)
    clean_cells = ctx.ndt_cells(T_, p)
    assert all(np.array_equal(dirty_cells[k], clean_cells[k]) for k in ("key", "count")) and np.isfinite(dirty_cells["icov"]).all()
    assert all(np.array_equal(bits(dirty_cells[k]), bits(clean_cells[k])) for k in ("mean", "icov"))
    prm = R.params(**case["prm"])
    for pose, d in zip(NC.poses(), dirty):
        c = ctx.ndt_sums(S, T_, p, pose)
        _, mag = R.sums(clean["src"], R.build_cells(clean["tgt"], prm), prm, pose, with_abs=True)
        assert np.isfinite(d).all() and d[27] == c[27] and (np.abs(d - c) <= SUM_TOL * mag).all()


def within_bars(A, B, what):
    dr, dt = np.abs(A[:3, :3] - B[:3, :3]).max(), np.abs(A[:3, 3] - B[:3, 3]).max()
    print("%s: rotation within %.2g, translation within %.2g" % (what, dr, dt))
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (what, dr, dt)


@pytest.fixture(scope="module")
def aligned(mvr, ctx, ref_cells):
    out = {}
    for case in NC.all_align_cases():
        prm = R.params(**case["prm"])
        load(ctx, case)
        got = ctx.ndt_align(S, T_, -1, mvr.ndt_params(**case["prm"]), case["G"], return_trace=True)
        out[case["name"]] = (case, got, R.align(case["src"], ref_cells(case), prm, case["G"]))
    return out


BRANCH_NAMES = ["fallback", "fallback-35", "fallback-2", "flat-0", "flat-1", "iterations"]


@pytest.mark.parametrize("name", [c + "-" + r for c in ("centred", "far", "guess") for r in ("res5", "res10")] + BRANCH_NAMES)
def test_align_follows_the_reference(aligned, name):
    """stop, iterations, evaluations and, iteration by iteration, trials and the reversed / fallback flags equal the reference's;
    a bit-equal where it is a halving of the cap (step_size), else within 1e-9; the score within 1e-9; X_out within the parity
    bars of the reference's; the residual against the known motion at most twice the reference's"""
    case, (T, X, st, rc, trace), ref = aligned[name]
    assert rc == 0 and (st["stop"], st["iterations"], st["evaluations"], st["converged"]) == (ref["stop"], ref["iterations"], ref["evaluations"], ref["converged"])
    assert len(trace) == len(ref["trace"])
    step = case["prm"]["step_size"]
    for k, (g, r) in enumerate(zip(trace, ref["trace"])):
        assert (g["trials"], g["reversed"], g["fallback"], g["stop"]) == (r["trials"], r["reversed"], r["fallback"], r["stop"]), (name, k, g, r)
        halving = r["a"] > 0 and np.log2(step / r["a"]) == np.round(np.log2(step / r["a"]))
        assert g["a"] == r["a"] if (halving or r["a"] == 0) else abs(g["a"] - r["a"]) <= 1e-9 * r["a"], (name, k, g["a"], r["a"])
        assert abs(g["delta_norm"] - r["delta_norm"]) <= 1e-8 * r["delta_norm"]
        assert abs(g["score"] - r["score"]) <= 1e-9 * abs(r["score"]) and np.abs(g["p"] - r["p"]).max() <= 1e-8
    assert abs(st["score"] - ref["score"]) <= 1e-9 * abs(ref["score"]) and st["n_pairs"] == ref["count"] and st["n_cells"] > 0
    within_bars(X, ref["X"], name)
    assert np.array_equal(T, X.astype(np.float32))
    mine, theirs = NC.residual(X, case), NC.residual(ref["X"], case)
    print("%s: %s after %d iterations, %d evaluations; residual %.4f (reference %.4f); %.2f ms" % (name, st["stop"], st["iterations"], st["evaluations"], mine, theirs, st["ms"]))
    assert mine <= 2 * theirs


def test_the_align_cases_reach_every_branch(aligned, mvr):
    """together the GPU's runs end on every stop and show both values of `reversed` and of `fallback`; each branch case takes
    the branch it was made for (the reference's trace, asserted in tests/test_ndt_host.py, is followed above)"""
    runs = [(st["stop"], trace) for _, (_, _, st, _, trace), _ in aligned.values()]
    assert NC.branches(runs) == NC.EVERY_BRANCH
    _, (T, X, st, rc, trace), _ = aligned["fallback"]
    assert rc == 0 and (st["stop"], st["converged"], st["iterations"], st["evaluations"]) == ("ITERATIONS", True, 1, 2)
    assert (trace[0]["trials"], trace[0]["reversed"], trace[0]["fallback"], trace[0]["a"]) == (1, True, True, NC.FALLBACK_STEP)
    assert np.array_equal(trace[0]["p"], [-NC.FALLBACK_STEP, 0, 0, 0, 0, 0]) and X[0, 3] == -NC.FALLBACK_STEP and st["score"] == trace[0]["score"]
    _, (_, _, st, rc, trace), _ = aligned["fallback-35"]
    assert rc == 0 and (st["stop"], st["converged"], st["iterations"], st["evaluations"]) == ("NO_DECREASE", False, 1, 3)
    assert [t["fallback"] for t in trace] == [True, False] and trace[1]["a"] == 0.0 and np.array_equal(trace[1]["p"], trace[0]["p"])
    _, (_, _, st, rc, trace), _ = aligned["fallback-2"]
    assert (st["stop"], st["iterations"], st["evaluations"], trace[0]["trials"], trace[0]["fallback"], trace[0]["a"]) == ("STEP", 1, 3, 2, False, NC.FALLBACK_STEP / 2)
    _, (T, X, st, rc, trace), _ = aligned["flat-0"]
    assert rc == 0 and (st["stop"], st["converged"], st["iterations"], st["evaluations"], st["n_pairs"], st["n_cells"]) == ("FLAT", False, 0, 1, 1, 1)
    assert np.array_equal(X, np.eye(4)) and np.array_equal(T, np.eye(4, dtype=np.float32)) and len(trace) == 1
    assert (trace[0]["a"], trace[0]["trials"], trace[0]["delta_norm"]) == (0.0, 0, 0.0)
    _, (T, X, st, rc, trace), _ = aligned["flat-1"]
    assert rc == 0 and (st["stop"], st["iterations"], st["evaluations"]) == ("FLAT", 1, 2) and X[0, 3] == -1.0 and [t["a"] for t in trace] == [1.0, 0.0]
    _, (_, _, st, rc, trace), _ = aligned["iterations"]
    _, (_, _, _, _, whole), _ = aligned["centred-res5"]
    assert (st["stop"], st["converged"], st["iterations"], st["evaluations"]) == ("ITERATIONS", True, 3, 5)
    for t, w in zip(trace, whole):            # the first three records are the uncut run's, bit for bit
        assert all(np.array_equal(t[k], w[k]) for k in ("a", "delta_norm", "trials", "reversed", "fallback", "score", "count", "p"))


def test_flat_with_a_guess_and_a_short_trace(mvr, ctx):
    """FLAT at the start returns the guess itself; a trace_cap shorter than the run cuts the trace and nothing else"""
    case = NC.one_cell("flat-guess", -0.5, step_size=1.0)
    case["prm"]["origin"] = (2.0, 2.0, 2.0)
    G = np.eye(4)
    G[0, 3] = 0.5                                                     # the guess puts the point on the cell's mean
    load(ctx, case)
    T, X, st, rc, trace = ctx.ndt_align(S, T_, -1, mvr.ndt_params(**case["prm"]), G, return_trace=True)
    assert rc == 0 and (st["stop"], st["iterations"], st["evaluations"]) == ("FLAT", 0, 1) and np.array_equal(X, G) and len(trace) == 1
    case = NC.branch_cases()[-1]
    load(ctx, case)
    p = mvr.ndt_params(**case["prm"])
    full = ctx.ndt_align(S, T_, -1, p, return_trace=True)
    for cap in (0, 1, 2):
        T, X, st, rc, trace = ctx.ndt_align(S, T_, -1, p, return_trace=True, trace_cap=cap)
        assert len(trace) == cap and np.array_equal(bits(X), bits(full[1])) and rc == full[3]
        assert {k: v for k, v in st.items() if k != "ms"} == {k: v for k, v in full[2].items() if k != "ms"}
        for t, w in zip(trace, full[4]):
            assert all(np.array_equal(t[k], w[k]) for k in t)


def test_far_equals_centred_and_guess_ends_where_centred_ends(aligned):
    for which in ("res5", "res10"):
        case, (_, Xc, stc, _, trc), _ = aligned["centred-" + which]
        _, (_, Xf, stf, _, trf), _ = aligned["far-" + which]
        _, (_, Xg, _, _, _), _ = aligned["guess-" + which]
        assert (stf["stop"], stf["iterations"], stf["evaluations"]) == (stc["stop"], stc["iterations"], stc["evaluations"])
        assert [(t["trials"], t["reversed"], t["fallback"]) for t in trf] == [(t["trials"], t["reversed"], t["fallback"]) for t in trc]
        within_bars(NC.far_to_centred(Xf), Xc, "far against centred, " + which)
        assert NC.residual(Xg, case) <= 2 * NC.residual(Xc, case)


def test_no_overlap_exit(mvr, ctx):
    case = NC.disjoint()
    load(ctx, case)
    p = mvr.ndt_params(**case["prm"])
    T, X, st, rc, trace = ctx.ndt_align(S, T_, -1, p, return_trace=True)
    assert rc == mvr.E_NOCORR and st["stop"] == "NO_OVERLAP" and not st["converged"] and (st["iterations"], st["evaluations"]) == (0, 1) and trace == []
    assert np.array_equal(X, np.eye(4)) and np.array_equal(T, np.eye(4, dtype=np.float32))
    G = R.pose_matrix(0.5 * NC.P_STAR)
    T, X, st, rc = ctx.ndt_align(S, T_, -1, p, G)
    assert rc == mvr.E_NOCORR and np.abs(X - G).max() <= 1e-15 and st["n_pairs"] == 0
    ctx.clear(S)                                                     # an empty source takes the same exit
    assert ctx.ndt_align(S, T_, -1, p)[3] == mvr.E_NOCORR
    load(ctx, case)
    ctx.upload(T_, case["tgt"][:5])                                  # ... and so does a target without a cell
    T, X, st, rc = ctx.ndt_align(S, T_, -1, p)
    assert rc == mvr.E_NOCORR and st["n_cells"] == 0 and st["stop"] == "NO_OVERLAP"


def test_nonfinite_align_equals_the_clean_one(mvr, ctx):
    case = NC.nonfinite()
    p = mvr.ndt_params(**case["prm"])
    load(ctx, case)
    T, X, st, rc, trace = ctx.ndt_align(S, T_, -1, p, return_trace=True)
    load(ctx, case["clean"])
    Tc, Xc, stc, rcc, tracec = ctx.ndt_align(S, T_, -1, p, return_trace=True)
    assert rc == rcc == 0 and np.isfinite(X).all()
    assert (st["stop"], st["iterations"], st["evaluations"], st["n_pairs"], st["n_cells"]) == (stc["stop"], stc["iterations"], stc["evaluations"], stc["n_pairs"], stc["n_cells"])
    assert [(t["trials"], t["reversed"], t["fallback"]) for t in trace] == [(t["trials"], t["reversed"], t["fallback"]) for t in tracec]
    within_bars(X, Xc, "nonfinite against clean")


def test_out_slot_and_inputs(mvr, ctx):
    case = NC.centred("res10")
    load(ctx, case)
    p = mvr.ndt_params(**case["prm"])
    T, X, st, rc = ctx.ndt_align(S, T_, O, p)
    assert rc == 0
    out = ctx.download(O)
    ctx.transform_f32(3, S, T)
    assert np.array_equal(out.view(np.uint32), ctx.download(3).view(np.uint32)) and len(out) == len(case["src"])
    assert np.array_equal(ctx.download(S).view(np.uint32), case["src"].view(np.uint32))
    assert np.array_equal(ctx.download(T_).view(np.uint32), case["tgt"].view(np.uint32))
    T2, X2, st2, _ = ctx.ndt_align(S, T_, -1, p)                        # bit-identical from run to run, with or without an output
    assert np.array_equal(bits(X), bits(X2)) and st["score"] == st2["score"]
    for bad in (S, T_):                                                 # N11: the output may be neither input
        with pytest.raises(mvr.MvrError) as e:
            ctx.ndt_align(S, T_, bad, p)
        assert e.value.status == mvr.E_ARG
