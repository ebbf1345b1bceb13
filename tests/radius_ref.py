"""numpy reference of the radius search (include/mvr_hip.h: mvr_radius_search, rules RS1-RS6), on top of the exact f32 distance of
tests/normals_ref.py / tests/outlier_ref.py: the d2 matrix of a chunk of queries, the mask finite & d2 <= float32(radius * radius),
the keys (bits(d2) << 32) | j, sorted, truncated to max_nn.  Returns CSR.

The fma arm of the distance is 80-bit arithmetic and slow, so it is spent on the pairs that can be listed only: both expressions
start from the same rounded differences and round three times, so they differ by less than 1e-6 relative (outlier_ref.within_r2)
-- a pair whose plain d2 is beyond r2 * (1 + 1e-6) is not listed under either, and every other pair gets the fma value."""
import numpy as np

import normals_ref as N
from outlier_ref import d2_f32

F32 = np.float32


def clamp_r2(radius):
    return F32(min(float(radius) * float(radius), float(np.finfo(F32).max)))


def radius_search(q, t, radius, max_nn=0, fma=False, chunk=None):
    """(offsets uint64[n + 1], idx uint32[total], d2 float32[total]): every row ascending under (d2, index)"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    n, m = len(q), len(t)
    r2 = clamp_r2(radius)
    chunk = chunk or max(1, int(2e7 // max(m, 1)))
    counts = np.zeros(n, np.uint64)
    keys_out = []
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        if m == 0:
            break
        D = N.dist2_f32(q[a:b], t, False)
        with np.errstate(invalid="ignore"):
            if fma:
                cand = np.isfinite(D) & (D.astype(np.float64) <= float(r2) * (1.0 + 1.0e-6))
                ii, jj = np.nonzero(cand)
                D = np.full(D.shape, np.inf, F32)
                if len(ii):
                    D[ii, jj] = d2_f32(q[a + ii, :3], t[jj, :3], True)
            mask = np.isfinite(D) & (D <= r2)
        # the keys of a row, the entries outside the ball last, sorted row by row
        K = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)[None, :]
        K[~mask] = np.uint64(0xFFFFFFFFFFFFFFFF)
        K.sort(axis=1)
        cnt = mask.sum(1)
        if max_nn:
            cnt = np.minimum(cnt, max_nn)
        keys = K[np.arange(m)[None, :] < cnt[:, None]]
        counts[a:b] = cnt
        keys_out.append(keys)
    keys = np.concatenate(keys_out) if keys_out else np.zeros(0, np.uint64)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(counts)
    return offsets, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32).view(F32)


def rows(offsets, idx):
    """the rows of a CSR result as a list of arrays"""
    o = offsets.astype(np.int64)
    return [idx[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def keys_of(idx, d2):
    return (np.ascontiguousarray(d2, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, np.uint32).astype(np.uint64)


def sort_rows(offsets, idx, d2):
    """the same lists with every row ordered by (d2, index): what an unordered result (RS5) is compared through"""
    o = offsets.astype(np.int64)
    owner = np.repeat(np.arange(len(o) - 1), np.diff(o))
    k = keys_of(idx, d2)
    order = np.lexsort((k, owner))
    return idx[order], d2[order]


def max_total_ok(total, long_records, ordered, bound=0x7FFFFFFF):
    """the arithmetic of rule RS8: the entries returned, and the keys of the long rows a call has to order, both fit the bound"""
    return total <= bound and not (ordered and long_records > bound)
