"""What the GPU tests of the moving-least-squares smoothing hold a result to, shared by tests/test_gpu_mls.py (the synthetic
views) and tests/test_gpu_mls_cases.py (the case table of tests/mls_cases.py): every coordinate, normal component and pinned
curvature within one f32 ulp of the f64 reference rounded to f32, at most DIFFER_CAP of the coordinates differing at all, and
the coplanar-curvature rule.  Plain numpy: no device is touched here."""
import numpy as np

import mls_ref as R

DIFFER_CAP = 1e-5          # share of the non-excluded coordinates that may differ at all (by one ulp)
FLAT = 1e-6                # curvature below which a neighbourhood counts as coplanar (l0 is then below 1e-6 of the trace)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def compare_values(what, got_xyz, got_nrm, got_curv, ref, bad, flat, zero=None):
    """bad: the kept points left out of every comparison; flat: those whose curvature alone is left out (coplanar
    neighbours, mls_ref.curvature_unpinned); zero: [kept, 3], the normal components the reference cannot pin to an f32 ulp
    (mls_ref.normal_unpinned: exactly 0 but for rounding noise) -- those, and only those, are held to 1e-9 absolute, the bar of
    the reference's own two routes"""
    ok = ~bad
    n_ok = int(ok.sum())
    one = R.within_one_ulp(got_xyz[ok], ref["xyz"][ok])
    differ = bits(got_xyz[ok]) != bits(ref["xyz"][ok])
    n1 = R.within_one_ulp(got_nrm[ok], ref["normal"][ok])
    if zero is not None:
        near = np.abs(got_nrm[ok].astype(np.float64) - ref["normal"][ok].astype(np.float64)) <= R.MAX_ROUTE_DIFF
        print("%s: %d normal components the reference cannot pin to an ulp (0 but for rounding), %d of them beyond one ulp, the "
              "largest of them %.3g" % (what, int(zero[ok].sum()), int((zero[ok] & ~n1).sum()),
                                        np.abs(ref["normal"][ok][zero[ok]]).max() if zero[ok].any() else 0.0))
        n1 = n1 | (zero[ok] & near)
        if not n1.all():
            print("%s: normal components beyond their bar (got, reference): %s"
                  % (what, list(zip(got_nrm[ok][~n1][:6].tolist(), ref["normal"][ok][~n1][:6].tolist()))))
    nd = bits(got_nrm[ok]) != bits(ref["normal"][ok])
    okc = ok & ~flat
    c1 = R.within_one_ulp(got_curv[okc], ref["curvature"][okc])
    cd = bits(got_curv[okc]) != bits(ref["curvature"][okc])
    print("%s: %d compared, %d excluded; coordinates beyond one ulp %d, differing %d of %d (share %.2e); normal components "
          "beyond one ulp %d, differing %d; curvatures beyond one ulp %d, differing %d, not pinned by the reference %d"
          % (what, n_ok, int(bad.sum()), int((~one).sum()), int(differ.sum()), differ.size, differ.mean() if differ.size else 0.0,
             int((~n1).sum()), int(nd.sum()), int((~c1).sum()), int(cd.sum()), int(flat.sum())))
    assert one.all() and n1.all() and c1.all()
    assert differ.mean() <= DIFFER_CAP
    # where the one-ulp check of the curvature is waived the neighbours are coplanar to rounding: the reference says so, and
    # what the GPU returns must say the same
    w = ok & flat
    assert (ref["curvature"][w] < FLAT).all() and (got_curv[w] >= 0).all() and (got_curv[w] < FLAT).all()
