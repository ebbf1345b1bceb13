"""shared inputs of the rejector tests (tests/test_reject_host.py on the CPU, tests/test_gpu_reject.py on the GPU).  Sizes are
chosen for the launch shapes of csrc/mvr_reject.hip: every kernel runs blocks of 256 threads (four waves of 64); the predicate,
histogram and one-to-one passes stride over the table with at most 1024 blocks; the trimmed stage gives each of at most 1024
blocks a range of whole 256-entry tiles; the select's scan walks 2048 bins, 8 per thread.  So 65 and 257 are a wave / a block
(= a tile) plus one, 6 001 is 23 tiles and a tail, 20 011 is 78 tiles and a tail, and BIG = 1024 x 256 + 257 entries (a
host list, no search: tests/test_gpu_reject.py) is where a block strides twice and a trimmed block takes two tiles.

A case is a pair of clouds (with normals or without), a search distance and the chains to run on it; every chain names the
`reciprocal` settings it is run under.  CONDITION, asserted by the host test on correspondences from an exhaustive numpy search:
in every case not named "degenerate..." each stage of each chain rejects at least one correspondence and keeps at least 3."""
import numpy as np

F32 = np.float32
BIG = 1024 * 256 + 257


def _pose(mvr, sp, view, pts, nrm=None):
    """the view under the turntable prior, computed here (f64, rounded once) so that the CPU sees the points the GPU gets"""
    piv, ax = mvr.synth_prior(sp)
    T = mvr.axis_rotation(piv, ax, mvr.turntable_angle(view, sp.n_views))
    out = pts.copy()
    out[:, :3] = (pts[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32)
    if nrm is None:
        return out
    n = nrm.copy()
    n[:, :3] = (nrm[:, :3].astype(np.float64) @ T[:3, :3].T).astype(F32)
    return out, n


def _synth_pair(mvr, ns, nt, normals=False, config=1):
    sp = mvr.synth_params(12, config)
    if not normals:
        return dict(src=_pose(mvr, sp, 1, mvr.synth_view(sp, 1, ns)), tgt=mvr.synth_view(sp, 0, nt))
    b, bn = mvr.synth_view(sp, 1, ns, normals=True)
    a, an = mvr.synth_view(sp, 0, nt, normals=True)
    b, bn = _pose(mvr, sp, 1, b, bn)
    return dict(src=b, tgt=a, snrm=bn, tnrm=an)


def _rand_pair(seed, ns, nt, scale=10.0):
    rng = np.random.default_rng(seed)

    def cloud(n):
        p = np.ones((n, 4), F32)
        p[:, :3] = (rng.standard_normal((n, 3)) * scale + (0.0, 0.0, 900.0)).astype(F32)
        return p
    return dict(src=cloud(ns), tgt=cloud(nt))


def _lattice_pair(seed=5, side=30):
    """target: the integer lattice (x, y, 0); source: the same (x, y) at a height of 0, 0.25, 0.5 or 0.75, so every d2 is one of four exact values and
    each value is taken hundreds of times: the median and the trimmed cut fall inside runs of equal distances"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    t = np.ones((side * side, 4), F32)
    t[:, 0], t[:, 1], t[:, 2] = gx.ravel(), gy.ravel(), 0.0
    s = t.copy()
    s[:, 2] = rng.integers(0, 4, len(s)) * 0.25           # heights 0, 0.25, 0.5, 0.75: exact in f32, below half the pitch
    o = rng.permutation(len(s))
    return dict(src=np.ascontiguousarray(s[o]), tgt=t)


def _shared_target_pair(seed=6, nt=40, per=15):
    """many sources around each of a few targets: without the reciprocal test most targets are matched many times"""
    rng = np.random.default_rng(seed)
    t = np.ones((nt, 4), F32)
    t[:, :3] = (rng.standard_normal((nt, 3)) * 50.0).astype(F32)
    s = np.repeat(t, per, axis=0)
    s[:, :3] += (rng.standard_normal((len(s), 3)) * 1.0).astype(F32)
    s[::7, :3] = s[1::7, :3][:len(s[::7])]                  # duplicates: equal distances to the same target, the lower index wins
    return dict(src=np.ascontiguousarray(s[rng.permutation(len(s))]), tgt=t)


DOT_EDGE = float(F32(0.6))                                 # a threshold some dots land on exactly: they fail (R5 is strict)


def _palette_normals(pair, seed=8):
    """source normals from a small palette, target normals all (1, 0, 0): the dots are exactly 1, 0.8f, 0.6f, 0 or NaN"""
    rng = np.random.default_rng(seed)
    pal = np.array([[1, 0, 0, 0], [0.8, 0.6, 0, 0], [0.6, 0.8, 0, 0], [0, 0, 1, 0], [np.nan, 0, 0, 0], [0.6, np.nan, 0, 0]], F32)
    out = dict(pair)
    out["snrm"] = pal[rng.integers(0, len(pal), len(pair["src"]))]
    out["tnrm"] = np.tile(np.array([1, 0, 0, 0], F32), (len(pair["tgt"]), 1))
    return out


BOTH, PLAIN = (0, 1), (0,)
_cases = {}


def build(mvr):
    """name -> dict(src, tgt[, snrm, tnrm], max_dist, chains = [(chain, reciprocal settings)])"""
    if _cases:
        return _cases
    c = _cases
    eight = [("distance", 1.9), ("median", 1.5), ("trimmed", 0.9), ("median", 1.3), ("trimmed", 0.9, 5), ("distance", 1.0), ("median", 1.2),
             ("trimmed", 0.75)]
    c["synth_6001"] = dict(_synth_pair(mvr, 6001, 5000), max_dist=4.0, chains=[
        ([("distance", 2.0)], BOTH), ([("median", 2.0)], BOTH), ([("trimmed", 0.8)], BOTH), ([("one_to_one",)], PLAIN),
        ([("median", 2.0), ("trimmed", 0.8)], BOTH), (eight, BOTH)])
    c["synth_20011"] = dict(_synth_pair(mvr, 20011, 6001), max_dist=4.0, chains=[
        ([("median", 2.0), ("trimmed", 0.8)], BOTH), ([("one_to_one",), ("trimmed", 0.5)], PLAIN)])
    c["synth_normals_6001"] = dict(_synth_pair(mvr, 6001, 6001, normals=True), max_dist=4.0, chains=[
        ([("surface_normal", 0.9995)], BOTH), ([("distance", 3.0), ("one_to_one",), ("surface_normal", 0.9995)], PLAIN)])
    c["synth_257"] = dict(_synth_pair(mvr, 257, 300), max_dist=40.0, chains=[
        ([("median", 1.0), ("trimmed", 0.5)], BOTH), ([("trimmed", 0.1, 20)], BOTH), ([("one_to_one",)], PLAIN)])
    c["rand_65"] = dict(_rand_pair(3, 65, 257), max_dist=30.0, chains=[
        ([("median", 1.0)], BOTH), ([("trimmed", 0.5)], BOTH), ([("distance", 5.0)], BOTH), ([("trimmed", 0.01, 7)], BOTH)])
    c["rand_257_palette"] = dict(_palette_normals(_rand_pair(4, 257, 65)), max_dist=30.0, chains=[
        ([("surface_normal", DOT_EDGE)], BOTH), ([("distance", 12.0), ("one_to_one",), ("surface_normal", DOT_EDGE)], PLAIN)])
    c["lattice"] = dict(_lattice_pair(), max_dist=2.0, chains=[
        ([("median", 1.0)], BOTH), ([("trimmed", 0.6)], BOTH), ([("median", 1.0), ("trimmed", 0.5)], BOTH), ([("trimmed", 0.1, 300)], BOTH)])
    c["shared_target"] = dict(_shared_target_pair(), max_dist=10.0, chains=[
        ([("one_to_one",)], PLAIN), ([("distance", 2.5), ("one_to_one",)], PLAIN), ([("one_to_one",), ("median", 1.0)], PLAIN)])
    # degenerate: stages that reject nothing, keep nothing, or meet an empty table
    c["degenerate_n1"] = dict(_rand_pair(11, 1, 5), max_dist=1e3, chains=[([("median", 1.0), ("trimmed", 0.5), ("one_to_one",)], BOTH)])
    c["degenerate_n2"] = dict(_rand_pair(12, 2, 5), max_dist=1e3, chains=[([("median", 1.0)], BOTH), ([("trimmed", 0.5)], BOTH)])
    c["degenerate_n3"] = dict(_rand_pair(13, 3, 2), max_dist=1e3, chains=[([("one_to_one",), ("median", 1.0)], BOTH), ([("trimmed", 0.4), ("median", 0.5)], BOTH)])
    c["degenerate_keep_all"] = dict(_rand_pair(14, 300, 300), max_dist=1e3, chains=[
        ([("trimmed", 1.0)], BOTH), ([("trimmed", 0.2, 100000)], BOTH), ([("trimmed", 7.5e9)], BOTH), ([("median", 1e9), ("distance", 1e9)], BOTH)])
    c["degenerate_empty_after"] = dict(_rand_pair(15, 300, 300), max_dist=1e3, chains=[
        ([("distance", 0.0), ("median", 2.0), ("trimmed", 0.5, 3), ("one_to_one",)], BOTH), ([("trimmed", 0.0), ("median", 1.0)], BOTH),
        ([("median", 0.0)], BOTH)])
    c["degenerate_no_match"] = dict(_rand_pair(16, 65, 65), max_dist=1e-3, chains=[([("median", 1.0), ("trimmed", 0.5)], BOTH)])
    return c


def runs(cases):
    return [(name, k) for name, case in cases.items() for k in range(len(case["chains"]))]


NAMES = ("synth_6001", "synth_20011", "synth_normals_6001", "synth_257", "rand_65", "rand_257_palette", "lattice", "shared_target",
         "degenerate_n1", "degenerate_n2", "degenerate_n3", "degenerate_keep_all", "degenerate_empty_after", "degenerate_no_match")
