"""shared inputs of the sample-consensus rejector's tests (tests/test_reject_sac_host.py on the CPU, tests/test_gpu_reject_sac.py
on the GPU).  Sizes follow the launch shapes of csrc/mvr_reject_sac.hip: blocks of 256 threads (four waves of 64), a counting
tile of 1024 pairs per block, strided passes of at most 1024 blocks.  So 65, 257 and 1025 pairs are a wave, a block and a tile
plus one, and reject_cases.BIG = 1024 x 256 + 257 pairs is where the strided passes go round twice.

A case is dict(src, tgt, q, m, d, value, max_iterations, refine, seed) plus
  planted   the indices (into the list sorted by query) a PLANTED case must keep, or None;
  check_c   True when check (c) of reject_sac_ref.verify is asserted on it (the reference then shows that >= 90 % of its
            counted attempts are well conditioned);
  found     what `found` must be."""
import math

import numpy as np

import reject_cases as RC

F32, F64 = np.float32, np.float64
THRESHOLD = 0.05          # PCL's default inlier threshold


def _motion(rng):
    """a rigid motion with a rotation of tens of degrees"""
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    ang = rng.uniform(0.3, 1.2)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    T[:3, 3] = rng.uniform(-2.0, 2.0, 3)
    return T


def _cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = xyz
    return p


def planted(n, seed, share=0.5, side=10.0, rej_seed=0, max_iterations=0, refine=False, check_c=True):
    """n pairs in [0, side)^3: `share` of them an exact rigid copy rounded to f32, the others matched to random targets; every
    source point is a query, the matches are a permutation of the targets"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.0, side, (n, 3)).astype(F32)
    T = _motion(rng)
    tgt_of = (src.astype(F64) @ T[:3, :3].T + T[:3, 3]).astype(F32)
    n_in = int(round(share * n))
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:n_in]] = True
    tgt_of[~inl] = rng.uniform(0.0, side, (n - n_in, 3)).astype(F32)
    perm = rng.permutation(n).astype(np.int32)
    tgt = np.empty((n, 3), F32)
    tgt[perm] = tgt_of
    q = np.arange(n, dtype=np.int32)
    d = ((src - tgt[perm]).astype(F32) ** 2).sum(1).astype(F32)
    return dict(src=_cloud(src), tgt=_cloud(tgt), q=q, m=perm, d=d, value=THRESHOLD, max_iterations=max_iterations, refine=refine, seed=rej_seed,
                planted=np.nonzero(inl)[0], check_c=check_c, found=True, motion=T)


def _unrelated(n, seed):
    rng = np.random.default_rng(seed)
    src, tgt = rng.uniform(0.0, 10.0, (n, 3)).astype(F32), rng.uniform(0.0, 10.0, (n, 3)).astype(F32)
    q = np.arange(n, dtype=np.int32)
    m = rng.permutation(n).astype(np.int32)
    d = ((src - tgt[m]) ** 2).sum(1).astype(F32)
    return dict(src=_cloud(src), tgt=_cloud(tgt), q=q, m=m, d=d, value=1e-4, max_iterations=70, refine=False, seed=5, planted=None, check_c=True,
                found=False)


def _non_finite(n, seed):
    """planted, with non-finite coordinates among the source points and the targets of some pairs, inliers and outliers alike"""
    c = planted(n, seed, check_c=True)
    rng = np.random.default_rng(seed + 1)
    bad_s, bad_t = rng.permutation(n)[:n // 8], rng.permutation(n)[:n // 8]
    vals = np.array([np.nan, np.inf, -np.inf], F32)
    c["src"][bad_s, rng.integers(0, 3, len(bad_s))] = vals[rng.integers(0, 3, len(bad_s))]
    c["tgt"][bad_t, rng.integers(0, 3, len(bad_t))] = vals[rng.integers(0, 3, len(bad_t))]
    ok = np.isfinite(c["src"][c["q"], :3]).all(1) & np.isfinite(c["tgt"][c["m"], :3]).all(1)
    c["planted"] = np.array([i for i in c["planted"] if ok[i]])
    return c


def _few_valid(seed):
    """ten pairs, two of them valid: no attempt, everything kept"""
    c = planted(10, seed, share=1.0)
    c["src"][2:, 0] = np.nan
    c.update(planted=None, found=False, check_c=False)
    return c


def _duplicates(n, seed):
    """planted, where every fifth source point (and its target) is an exact copy of one of four points: samples with two or
    three equal pairs, whose covariance has rank 1 or 0"""
    c = planted(n, seed, share=1.0, check_c=False)
    for k in range(0, n, 5):
        c["src"][k] = c["src"][k % 4]
        c["tgt"][c["m"][k]] = c["tgt"][c["m"][k % 4]]
    c["d"] = ((c["src"][:, :3] - c["tgt"][c["m"], :3]) ** 2).sum(1).astype(F32)
    c["planted"] = np.arange(n)
    return c


def _sparse(seed):
    """a caller's list that names a subset of the source points, in no order: 300 of 1025"""
    c = planted(1025, seed)
    rng = np.random.default_rng(seed + 2)
    pick = rng.permutation(1025)[:300]
    pos = {int(i): k for k, i in enumerate(np.sort(pick))}
    c["planted"] = np.array(sorted(pos[int(i)] for i in pick if i in set(c["planted"].tolist())))
    c.update(q=c["q"][pick], m=c["m"][pick], d=c["d"][pick])
    return c


_cases = {}
NAMES = ("empty", "two", "three", "planted_65", "planted_257", "planted_1025", "planted_1500", "planted_1500_refine", "planted_30",
         "all_inliers", "unrelated", "non_finite", "few_valid", "duplicates", "sparse_shuffled", "big")
HOST_NAMES = tuple(n for n in NAMES if n != "big")      # (the host test leaves the quarter of a million pairs to the GPU)


def build():
    """name -> case.  The committed seeds are chosen so that the reference keeps exactly the planted pairs and no stop decision of
    the loop lies within sac_ref.K_MARGIN of k (tests/test_reject_sac_host.py asserts both)."""
    if _cases:
        return _cases
    c = _cases
    c["empty"] = dict(planted(16, 1), q=np.zeros(0, np.int32), m=np.zeros(0, np.int32), d=np.zeros(0, F32), planted=None, found=False, check_c=False)
    two = planted(16, 2)
    c["two"] = dict(two, q=two["q"][[9, 3]], m=two["m"][[9, 3]], d=two["d"][[9, 3]], planted=None, found=False, check_c=False)
    c["three"] = planted(3, 3, share=1.0, check_c=False)
    c["planted_65"] = planted(65, 4, rej_seed=1)
    c["planted_257"] = planted(257, 5, rej_seed=2)
    c["planted_1025"] = planted(1025, 6, rej_seed=3)
    c["planted_1500"] = planted(1500, 7, rej_seed=4)
    c["planted_1500_refine"] = planted(1500, 7, rej_seed=4, refine=True)
    c["planted_30"] = planted(2000, 8, share=0.3, rej_seed=6, refine=True)
    c["all_inliers"] = planted(300, 9, share=1.0, rej_seed=7)
    c["unrelated"] = _unrelated(400, 10)
    c["non_finite"] = _non_finite(257, 11)
    c["few_valid"] = _few_valid(12)
    c["duplicates"] = _duplicates(200, 13)
    c["sparse_shuffled"] = _sparse(14)
    c["big"] = planted(RC.BIG, 15, rej_seed=8)
    return c


def shuffled(case, seed=99):
    """the same list in another order"""
    o = np.random.default_rng(seed).permutation(len(case["q"]))
    return dict(case, q=case["q"][o], m=case["m"][o], d=case["d"][o])
