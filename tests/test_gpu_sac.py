"""GPU tests of the plane segmentation (mvr_cloud_segment_plane, mvr_cloud_extract_indices; rules P1-P12 in include/mvr_hip.h)
against the numpy reference of tests/sac_ref.py on the inputs of tests/sac_cases.py.

The RANSAC stage is claimed EXACT, not within a tolerance: draws are integer arithmetic, the model and the distance are f32
operations rounded one by one in a fixed order (sqrtf and the division are correctly rounded under the project's flags), the
counts are integers.  So the whole trace -- statuses, samples, coefficient bits, counts --, the loop's outcome, the RANSAC plane
and its inlier set are compared bit for bit; k alone goes through libm's log and is compared to a relative 1e-12 (the cases
keep every stop decision 0.01 away from it).

The refinement (P10) goes through the library's Jacobi where the reference uses eigh, so the f64 plane BEFORE the cast to f32
is compared within sac_ref's measured bars: a component n_c of a unit normal moves by at most the angle the normal turns by, so
the GPU's f32 n_c must lie in [f32(n_c - bar), f32(n_c + bar)] of the reference's, and its d in [f32(d - bar_d), f32(d + bar_d)]:
the values the cast can give from an f64 plane within the bars.  The refined inlier set is then compared exactly, with P5
recomputed on the host from the GPU's own refined coefficients."""
import importlib

import numpy as np
import pytest

import sac_cases as SC
import sac_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MODEL = {R.PLANE: "plane", R.PERPENDICULAR: "perpendicular_plane"}


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def call(ctx, dst, src, kw, seed, **more):
    a = dict(kw, **more)
    return ctx.segment_plane(dst, src, a["threshold"], model=MODEL[a.get("model", R.PLANE)], max_iterations=a.get("max_iterations", 1000),
                             probability=a.get("probability", 0.99), optimize=a.get("optimize", True), axis=a.get("axis"),
                             eps_angle=a.get("eps_angle"), seed=seed, negative=a.get("negative", False), fma=a.get("fma", False),
                             return_index=True, return_trace=True)


_gpu = {}


def gpu_run(ctx, name, seed=1, fma=False, optimize=True):
    key = (name, seed, fma, optimize)
    if key not in _gpu:
        p, kw, ref = SC.reference(name, seed, fma, optimize)
        ctx.upload(0, p)
        _gpu[key] = (p, kw, ref) + call(ctx, -1, 0, kw, seed, fma=fma, optimize=optimize)
        assert same_bits(ctx.download(0), p)                                 # dst = -1: the source is left as it was
    return _gpu[key]


def same_result(a, b):
    (ra, ia, ta), (rb, ib, tb) = a, b
    return (all(same_bits(ra[k], rb[k]) if isinstance(ra[k], np.ndarray) else ra[k] == rb[k] for k in ra) and np.array_equal(ia, ib)
            and all(same_bits(ta[k], tb[k]) for k in ta))


# ------------------------------------------------------------------ the RANSAC stage, exactly

@pytest.mark.parametrize("name,seed", SC.RUNS, ids=SC.IDS)
def test_trace_loop_and_ransac_plane_equal_the_references(name, seed, ctx):
    p, kw, ref, res, idx, tr = gpu_run(ctx, name, seed, optimize=False)
    rt = ref["trace"]
    print("%s seed %d: %d attempts (%d counted, %d skipped), best %d with %d inliers; reference %d / %d / %d / %d with %d"
          % (name, seed, res["attempts"], res["iterations"], res["skipped"], res["best_attempt"], res["inliers"], ref["attempts"],
             ref["iterations"], ref["skipped"], ref["best_attempt"], ref["ransac_mask"].sum()))
    assert len(tr["status"]) == res["attempts"] == ref["attempts"]
    assert np.array_equal(tr["status"], rt["status"]) and np.array_equal(tr["sample"], rt["sample"])
    assert same_bits(tr["coefficients"], rt["coefficients"])
    assert np.array_equal(tr["inliers"], rt["inliers"])
    assert (res["found"], res["iterations"], res["skipped"], res["best_attempt"]) == (ref["found"], ref["iterations"], ref["skipped"], ref["best_attempt"])
    assert np.allclose(tr["k"], rt["k"], rtol=1e-12, atol=0) and abs(res["k"] - ref["k"]) <= 1e-12 * abs(ref["k"])
    assert same_bits(res["ransac_coefficients"], ref["ransac_coefficients"]) and same_bits(res["coefficients"], ref["ransac_coefficients"])
    assert res["ransac_inliers"] == res["inliers"] == int(ref["ransac_mask"].sum()) == res["n_out"]
    assert np.array_equal(idx, np.nonzero(ref["ransac_mask"])[0]) and idx.dtype == np.uint32


def test_fma_distance(ctx):
    """on the far frame (coordinates of 1e4 mm, products of 1e4 rounded to 1e-3) the fma chain counts differently: the GPU with
    fma_dist must equal the fma reference where that differs from the plain one, and without it the plain one"""
    plain = SC.reference(SC.FMA_CASE, 1, False, False)[2]
    p, kw, ref, res, idx, tr = gpu_run(ctx, SC.FMA_CASE, 1, fma=True, optimize=False)
    differ = int((ref["trace"]["inliers"] != plain["trace"]["inliers"]).sum())
    print("fma changes %d of %d counts and %d entries of the inlier mask" % (differ, len(tr["inliers"]), (ref["ransac_mask"] != plain["ransac_mask"]).sum()))
    assert len(ref["trace"]["inliers"]) == len(plain["trace"]["inliers"]) and differ >= 1                # ransac_count_kernel<PlaneModel, ., true>
    assert (ref["ransac_mask"] != plain["ransac_mask"]).any()                                              # sac_flag_kernel<true>
    assert same_bits(tr["coefficients"], ref["trace"]["coefficients"]) and np.array_equal(tr["inliers"], ref["trace"]["inliers"])
    assert (res["iterations"], res["best_attempt"], res["inliers"]) == (ref["iterations"], ref["best_attempt"], int(ref["ransac_mask"].sum()))
    assert np.array_equal(idx, np.nonzero(ref["ransac_mask"])[0])
    _, _, _, res0, idx0, tr0 = gpu_run(ctx, SC.FMA_CASE, 1, fma=False, optimize=False)
    assert np.array_equal(tr0["inliers"], plain["trace"]["inliers"]) and np.array_equal(idx0, np.nonzero(plain["ransac_mask"])[0])
    # every register count of the counting kernel with fma: chunks of up to 64, 128 and 256 attempts, on a case with many attempts
    q, kq, rq = SC.reference("mostly_object", 1, True, False)
    ctx.upload(0, q)
    try:
        for chunk in (64, 128, 256):
            ctx.tune(sac_chunk=chunk)
            r, i, t = call(ctx, -1, 0, kq, 1, fma=True, optimize=False)
            assert np.array_equal(t["inliers"], rq["trace"]["inliers"]) and np.array_equal(i, np.nonzero(rq["ransac_mask"])[0]), chunk
    finally:
        ctx.tune(sac_chunk=0)


@pytest.mark.parametrize("name", ["mostly_object", "platter", "perpendicular", "collinear", "duplicates", "two_planes"])
def test_every_chunk_size_gives_the_same_bits(name, ctx):
    p, kw, ref = SC.reference(name)
    ctx.upload(0, p)
    got = {}
    try:
        for chunk in (1, 7, 64, 200, 0):
            ctx.tune(sac_chunk=chunk)
            got[chunk] = call(ctx, -1, 0, kw, 1)
    finally:
        ctx.tune(sac_chunk=0)
    for chunk in (1, 7, 64, 200):
        assert same_result(got[chunk], got[0]), chunk
    assert got[0][0]["attempts"] == ref["attempts"]


def test_run_to_run_identity(ctx):
    for name in ("platter", "far", "perpendicular"):
        p, kw, ref = SC.reference(name)
        ctx.upload(0, p)
        a, b = call(ctx, -1, 0, kw, 1), call(ctx, -1, 0, kw, 1)
        assert same_result(a, b) and a[0]["found"]


# ------------------------------------------------------------------ the refinement

@pytest.mark.parametrize("name", SC.FOUND)
def test_refined_plane_against_eigh_and_its_inliers_exactly(name, ctx):
    p, kw, ref, res, idx, tr = gpu_run(ctx, name)
    co = res["coefficients"]
    assert res["found"] and same_bits(res["ransac_coefficients"], ref["ransac_coefficients"]) and res["ransac_inliers"] == ref["ransac_mask"].sum()
    if ref["refined"] is None:
        assert same_bits(co, ref["ransac_coefficients"])
    elif name in SC.REFINED:
        nrm, d = ref["refined"]
        ang = R.angle_between(co[:3].astype(F64), nrm)
        print("%s: refined normal %.2e rad from the reference's (f32 against f64), d %.3e apart" % (name, ang, abs(float(co[3]) - d)))
        for c in range(3):
            assert F32(nrm[c] - R.REFINE_ANGLE_BAR) <= co[c] <= F32(nrm[c] + R.REFINE_ANGLE_BAR), (c, co, nrm)
        assert F32(d - R.REFINE_D_BAR) <= co[3] <= F32(d + R.REFINE_D_BAR), (co, d)
        assert float(co[:3].astype(F64) @ ref["ransac_coefficients"][:3].astype(F64)) >= 0          # P10's orientation
    assert co.dtype == F32 and np.isfinite(co).all()
    mask = R.inlier_mask(co, p, kw["threshold"])
    assert np.array_equal(idx, np.nonzero(mask)[0]) and res["inliers"] == mask.sum() == res["n_out"]


# ------------------------------------------------------------------ the output (P11)

def normals_for(p):
    n = np.zeros((len(p), 4), F32)
    n[:, :3] = np.arange(3 * len(p), dtype=F32).reshape(-1, 3)               # any values: they must follow their points
    return n


@pytest.mark.parametrize("name", ["platter", "invalid_mixed", "collinear", "small"])
@pytest.mark.parametrize("negative", [False, True], ids=["inliers", "negative"])
def test_dst_contents(name, negative, ctx):
    p, kw, ref, res0, idx0, _ = gpu_run(ctx, name)
    nrm = normals_for(p)
    mask = np.zeros(len(p), bool)
    mask[idx0] = True
    keep = ~mask if negative else mask
    for dst in (1, 0):                                                       # another slot, then in place
        ctx.upload(0, p)
        ctx.upload_normals(0, nrm)
        res, idx, _ = call(ctx, dst, 0, kw, 1, negative=negative)
        assert np.array_equal(idx, idx0) and res["n_out"] == keep.sum() == ctx.size(dst) and res["inliers"] == mask.sum()
        assert same_bits(ctx.download(dst), p[keep])
        if keep.any():
            assert same_bits(ctx.download_normals(dst), nrm[keep])
        if dst != 0:
            assert same_bits(ctx.download(0), p) and same_bits(ctx.download_normals(0), nrm)
    if name == "invalid_mixed":
        bad = ~ref["valid"]
        assert bad.sum() > 0 and not mask[bad].any() and (keep[bad].all() if negative else not keep[bad].any())
    if name == "collinear":
        assert not res0["found"] and keep.sum() == (len(p) if negative else 0)


@pytest.mark.parametrize("name", ["n0", "n1", "n2", "all_invalid"])
def test_nothing_to_find(name, ctx):
    p, kw, ref, res, idx, tr = gpu_run(ctx, name)
    assert not res["found"] and res["attempts"] == 0 and res["inliers"] == 0 and len(idx) == 0 and len(tr["status"]) == 0 and res["k"] == 1.0
    assert res["best_attempt"] == -1 and not res["coefficients"].any()
    ctx.upload(0, p)
    ctx.upload(1, SC.CASES["small"][0])
    assert call(ctx, 1, 0, kw, 1)[0]["n_out"] == 0 and ctx.size(1) == 0
    assert call(ctx, 1, 0, kw, 1, negative=True)[0]["n_out"] == len(p) and same_bits(ctx.download(1), p)


def test_extract_indices(ctx):
    p = SC.CASES["invalid_mixed"][0]
    nrm = normals_for(p)
    rng = np.random.default_rng(5)
    pick = rng.choice(len(p), 300, replace=True).astype(np.uint32)           # unsorted, with repeats
    mask = np.zeros(len(p), bool)
    mask[pick] = True
    for negative in (False, True):
        keep = ~mask if negative else mask
        for dst in (1, 0):
            ctx.upload(0, p)
            ctx.upload_normals(0, nrm)
            assert ctx.extract_indices(dst, 0, pick, negative=negative) == keep.sum() == ctx.size(dst)
            assert same_bits(ctx.download(dst), p[keep]) and same_bits(ctx.download_normals(dst), nrm[keep])
    ctx.upload(0, p)
    assert ctx.extract_indices(1, 0, np.zeros(0, np.uint32)) == 0 and ctx.extract_indices(1, 0, [], negative=True) == len(p)
    with pytest.raises(Exception):
        ctx.extract_indices(1, 0, [len(p)])
    assert ctx.size(0) == len(p)
