"""A reference for mvr_cloud_denoise that is not the kernel's twin: no grid, no union-find.  Every pair of points is formed by
brute force in row blocks, d = sqrt(dx*dx + dy*dy + dz*dz) in f64 from the f32 coordinates (each operation rounded, in that
order: numpy fuses nothing), a pair is linked when `not (d > r)`, and scipy.sparse.csgraph.connected_components takes the
components.  A component's label is its smallest index, the components with size >= max(threshold, 0) are kept, and the output
is ordered by (label, index) -- the rule of include/mvr_hip.h, non-finite points included: a point with a non-finite x, y or z
is linked to nothing, so it is a component of its own (counted, kept exactly when threshold <= 1, at its place in the order).

The distances of a cloud do not depend on the radius, so components() takes a list of radii and forms each block once."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

BLOCK = 256


def components(pts, radii, margins=False):
    """{r: (label, n_components, margin)} for every r of `radii`: label[i] is the smallest index of point i's component.
    margin (with margins=True, else None): the smallest |d - r| / r over all pairs i != j of finite points, inf when there is
    no such pair or r is 0 or infinite."""
    radii = [float(r) for r in radii]
    n = len(pts)
    P = np.ascontiguousarray(pts[:, :3]).astype(np.float64)
    fin = np.isfinite(pts[:, :3]).all(1)
    rows = {r: [] for r in radii}
    margin = {r: np.inf for r in radii}
    for a in range(0, n, BLOCK):
        b = min(a + BLOCK, n)                    # rows a..b against the columns 0..b: every pair {i, j} once (and i == j)
        with np.errstate(invalid="ignore", over="ignore"):
            dx = P[a:b, None, 0] - P[None, :b, 0]
            dy = P[a:b, None, 1] - P[None, :b, 1]
            dz = P[a:b, None, 2] - P[None, :b, 2]
            d = np.sqrt(dx * dx + dy * dy + dz * dz)
        both = fin[a:b, None] & fin[None, :b]
        both &= np.arange(a, b)[:, None] > np.arange(b)[None, :]
        for r in radii:
            with np.errstate(invalid="ignore"):
                link = ~(d > r)
            link &= both
            m = sp.csr_matrix(link)
            m.resize(b - a, n)
            rows[r].append(m)
            if margins and np.isfinite(r) and r > 0 and both.any():
                margin[r] = min(margin[r], float((np.abs(d[both] - r) / r).min()))
    out = {}
    for r in radii:
        if n == 0:
            out[r] = (np.zeros(0, np.int64), 0, np.inf if margins else None)
            continue
        ncomp, lab = connected_components(sp.vstack(rows[r], format="csr"), directed=False)
        first = np.full(ncomp, n, np.int64)
        np.minimum.at(first, lab, np.arange(n))
        out[r] = (first[lab], int(ncomp), margin[r] if margins else None)
    return out


def select(label, threshold):
    """the kept indices in output order: components with size >= max(threshold, 0), ordered by (label, index)"""
    n = len(label)
    if n == 0:
        return np.zeros(0, np.uint32)
    size = np.bincount(label, minlength=n)
    order = np.lexsort((np.arange(n), label))
    return order[size[label[order]] >= max(int(threshold), 0)].astype(np.uint32)


def denoise(pts, threshold, r):
    """(kept indices in output order, label per point, number of components), as oracle.denoise returns them"""
    label, ncomp, _ = components(pts, [r])[float(r)]
    return select(label, threshold), label.astype(np.uint32), ncomp
