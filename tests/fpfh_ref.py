"""FPFH in numpy, fp64, vectorised: the reference that both sets of FPFH kernels (features.hip, coarse_batch.hip) and the C
oracle are compared with.  A restatement of PCL 1.7 FPFHEstimation (features/impl/fpfh.hpp) and computePairFeatures
(features/src/pfh.cpp), written from their text; it shares no code and no arithmetic with the kernels or with oracle/features.c.

The rules, all of them (DESIGN.md §2 repeats the ones that are not obvious from PCL's text):

Neighbourhood.  The neighbourhood of point i is every finite point j with |p_i - p_j|^2 <= r2, r2 = float32(r) * float32(r), the
    squared distance computed in fp64 from the fp32 coordinates.  It includes i itself; m_i is its size.  A non-finite point
    belongs to no neighbourhood and its row is NaN.

SPFH of i.  For every neighbour j != i BY INDEX (a duplicate of i is a neighbour like any other): computePairFeatures(p_i, n_i,
    p_j, n_j).  With d = p_j - p_i, f4 = |d|, a1 = n_i.d / f4, a2 = n_j.d / f4: the point whose normal makes the smaller angle
    with the line is the source, i.e. the roles are swapped (and d negated) if acos|a1| > acos|a2|; f3 = a1, or -a2 after a swap;
    v = (d x n_s) / |d x n_s|, w = n_s x v, f2 = v.n_t, f1 = atan2(w.n_t, n_s.n_t).  A pair is rejected only if f4 == 0 or
    |d x n_s| == 0.  These are comparisons and so is the swap: all three are false for NaN (a NaN normal rejects nothing and swaps
    nothing).

Binning.  floor(11 (f1 + pi) / (2 pi)), floor(11 (f2 + 1) / 2), floor(11 (f3 + 1) / 2), clamped to 0..10.  A non-finite feature goes
    to bin 0 of its own group, feature by feature: PCL's (int)floor(NaN) is INT_MIN on x86 and the clamp that follows makes it 0.
    (So a point whose own normal is NaN has the SPFH row [100, 0, ...] in each group if it has any neighbour but itself.)

Bin increment.  Every accepted pair adds hist_incr = 100 / (m_i - 1), a float, to one float bin per group: a bin that took c
    pairs holds the result of c float additions of hist_incr (np.cumsum of a float32 array), not c * hist_incr.  That is PCL's
    arithmetic and part of the specification.  (increments="fp64" replaces it by the exact c * 100 / (m_i - 1): what the loop
    fpfh_numpy of test_oracle_independent.py computes, for the cross-check with it.)

FPFH of i.  sum of spfh_j / d2_ij over the neighbours with d2_ij != 0 (i itself and its duplicates are left out; the weight is
    one over the SQUARED distance), then each 11-bin group is scaled to sum to 100; a group whose sum is 0 stays 0.  A finite
    point with only itself (and duplicates) in range gets a zero row.

fpfh_ref returns (fpfh (n, 33) fp64, spfh (n, 33) fp64, m (n,) int64, fragile (n,) bool).  A pair is fragile if one of its three bin
coordinates (the argument of floor above) lies within 1e-5 bin units of an interior bin edge 1..10, or if its fp64 squared
distance lies within 1e-6 relative of r2 (pairs just outside r2 too).  The distance test is skipped with exact=True: for clouds
whose coordinates are small multiples of a power of two, so that the fp32 squared distance is exact.  A row is fragile if any pair of
its own neighbourhood, or of a neighbour's neighbourhood, is fragile: fp32 arithmetic may put such a pair in another bin, or on
the other side of the radius, and the rows that see it move by whole increments.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.spatial import cKDTree

BIN_EDGE_TOL = 1e-5      # bin units
RADIUS_TOL = 1e-6        # relative, of r2


def _dot(a, b):
    return (a * b).sum(1)


def darboux_features(ps, ns, pt, nt):
    """The features of a pair whose source is (ps, ns): (f1, f2, f3, |d x ns|, |d|)."""
    with np.errstate(all="ignore"):
        d = pt - ps
        f4 = np.sqrt(_dot(d, d))
        f3 = _dot(ns, d) / f4
        v = np.cross(d, ns)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = np.cross(ns, v)
        f2 = _dot(v, nt)
        f1 = np.arctan2(_dot(w, nt), _dot(ns, nt))
    return f1, f2, f3, vn, f4


def swap_test(p1, n1, p2, n2):
    """acos|a1| > acos|a2| (False where either side is NaN), and the difference of the two angles."""
    with np.errstate(all="ignore"):
        d = p2 - p1
        f4 = np.sqrt(_dot(d, d))
        margin = np.arccos(np.abs(_dot(n1, d) / f4)) - np.arccos(np.abs(_dot(n2, d) / f4))
        return margin > 0, margin


def pair_features(p1, n1, p2, n2):
    """computePairFeatures for arrays of pairs (fp64): (f1, f2, f3, accepted)."""
    swap, _ = swap_test(p1, n1, p2, n2)
    s = swap[:, None]
    f1, f2, f3, vn, f4 = darboux_features(np.where(s, p2, p1), np.where(s, n2, n1), np.where(s, p1, p2), np.where(s, n1, n2))
    return f1, f2, f3, ~(f4 == 0) & ~(vn == 0)


def bin_coordinates(f1, f2, f3):
    """The arguments of floor(): (k, 3) bin coordinates in 0..11."""
    return np.stack([11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0], 1)


def bins_of(x):
    with np.errstate(invalid="ignore"):
        b = np.clip(np.floor(x), 0, 10)
    return np.where(np.isfinite(x), b, 0).astype(np.int64)


def neighbour_pairs(P64, finite, r2, slack=1e-4):
    """Directed pairs (I, J, d2), i != j, of finite points whose fp64 squared distance is <= r2 * (1 + slack): candidates from a
    kd-tree with a slightly larger radius, the distance recomputed exactly."""
    ids = np.flatnonzero(finite)
    if len(ids) < 2:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0)
    tree = cKDTree(P64[ids])
    pr = tree.query_pairs(np.sqrt(r2) * (1.0 + slack) + 1e-12, output_type="ndarray")
    a, b = ids[pr[:, 0]], ids[pr[:, 1]]
    d = P64[a] - P64[b]
    d2 = _dot(d, d)
    keep = d2 <= r2 * (1.0 + slack)
    a, b, d2 = a[keep], b[keep], d2[keep]
    return np.r_[a, b], np.r_[b, a], np.r_[d2, d2]


def _pairs(P, N, r, exact, touching=None):
    """Everything about the pairs of a cloud: the candidate pairs (Ic, Jc, d2c) out to a little beyond r2, which of them are inside
    and which within RADIUS_TOL of r2, the features and bin coordinates of the pairs inside, and own[i] = point i has a fragile pair.
    touching: a mask of points; only the pairs with one of them at either end are looked at."""
    P64 = np.ascontiguousarray(P, np.float32).astype(np.float64)
    N64 = np.ascontiguousarray(N, np.float32).astype(np.float64)
    n = len(P64)
    r2 = float(np.float32(r) * np.float32(r))
    finite = np.isfinite(P64).all(1)
    Ic, Jc, d2c = neighbour_pairs(P64, finite, r2)
    if touching is not None:
        sel = touching[Ic] | touching[Jc]
        Ic, Jc, d2c = Ic[sel], Jc[sel], d2c[sel]
    near_r = np.abs(d2c - r2) <= RADIUS_TOL * r2 if not exact else np.zeros(len(d2c), bool)
    inside = d2c <= r2
    I, J, d2 = Ic[inside], Jc[inside], d2c[inside]
    f1, f2, f3, ok = pair_features(P64[I], N64[I], P64[J], N64[J])
    x = bin_coordinates(f1, f2, f3)
    with np.errstate(invalid="ignore"):
        edge = np.rint(x)
        on_edge = ((np.abs(x - edge) < BIN_EDGE_TOL) & (edge >= 1) & (edge <= 10)).any(1) & ok
    own = np.zeros(n, bool)
    own[I[on_edge]] = True
    own[Ic[near_r]] = True
    return dict(n=n, finite=finite, Ic=Ic, Jc=Jc, inside=inside, near_r=near_r, I=I, J=J, d2=d2, ok=ok, x=x, own=own)


def unsettled_points(P, N, r, exact=False, touching=None):
    """The points with a pair of their own that is fragile (fpfh_ref) or undefined (undefined_rows)."""
    q = _pairs(P, N, r, exact, touching)
    return q["own"] | undefined_rows(P, N, r, own_only=True, q=q)


def undefined_rows(P, N, r, tol=1e-6, own_only=False, q=None):
    """Rows that no reference can judge: they see (in their own neighbourhood or a neighbour's) a pair whose features the rules
    above leave to rounding, whatever the precision, by more than a bin edge:
      - acos|a1| and acos|a2| within `tol` of each other, where the swap moves the pair to other bins (two normals with the same
        bits excepted: a1 and a2 are then the same number in any arithmetic, and nothing is swapped);
      - both arguments of atan2 below `tol` (n_s . n_t and w . n_t: f1 is any angle);
      - 0 < |d x n_s| < tol |d| (the normal along the line: v is any direction, and `== 0` may or may not reject the pair).
    No case of fpfh_cases.py has such a row (test_fpfh_ref.py).  The k-NN normals of a lattice, which the batch path computes for
    itself, are full of them: they are parallel, perpendicular and mirror images of one another, exactly.
    own_only: the points that have such a pair themselves."""
    q = _pairs(P, N, r, True) if q is None else q
    I, J, ok = q["I"], q["J"], q["ok"]
    P64 = np.ascontiguousarray(P, np.float32).astype(np.float64)
    N64 = np.ascontiguousarray(N, np.float32).astype(np.float64)
    p1, n1, p2, n2 = P64[I], N64[I], P64[J], N64[J]
    swap, margin = swap_test(p1, n1, p2, n2)
    s = swap[:, None]
    ps, ns, pt, nt = np.where(s, p2, p1), np.where(s, n2, n1), np.where(s, p1, p2), np.where(s, n1, n2)
    with np.errstate(all="ignore"):
        g1, g2, g3, _, _ = darboux_features(pt, nt, ps, ns)              # the roles the other way round
        tie = (np.abs(margin) < tol) & (bins_of(bin_coordinates(g1, g2, g3)) != bins_of(q["x"])).any(1) & (n1 != n2).any(1)
        d = pt - ps
        v = np.cross(d, ns)
        vn, f4 = np.sqrt(_dot(v, v)), np.sqrt(_dot(d, d))
        w = np.cross(ns, v / vn[:, None])
        free_angle = np.hypot(_dot(w, nt), _dot(ns, nt)) < tol
        along = (vn > 0) & (vn < tol * f4)
    bad = (tie | free_angle | along) & ok
    own = np.zeros(q["n"], bool)
    own[I[bad]] = True
    if own_only:
        return own
    rows = own.copy()
    rows[I[own[J]]] = True
    return rows


def fpfh_ref(P, N, r, exact=False, increments="pcl"):
    q = _pairs(P, N, r, exact)
    n, finite, I, J, d2, ok, x = q["n"], q["finite"], q["I"], q["J"], q["d2"], q["ok"], q["x"]
    m = np.bincount(I, minlength=n) + finite.astype(np.int64)

    # ---- SPFH
    b = bins_of(x)
    counts = np.zeros((n, 33), np.int64)
    for g in range(3):
        np.add.at(counts, (I[ok], 11 * g + b[ok, g]), 1)
    with np.errstate(divide="ignore"):
        if increments == "pcl":
            inc = (np.float32(100.0) / (m - 1).astype(np.float32)).astype(np.float32)
            cmax = int(counts.max()) if counts.size else 0
            # table[i, c] = the float that c additions of inc[i] leave (np.cumsum adds in sequence, in float32)
            table = np.zeros((n, cmax + 1), np.float32)
            if cmax:
                table[:, 1:] = np.cumsum(np.broadcast_to(inc[:, None], (n, cmax)), axis=1, dtype=np.float32)
            spfh = np.take_along_axis(table, counts, 1).astype(np.float64)
        elif increments == "fp64":
            spfh = counts * (100.0 / np.maximum(m - 1, 1))[:, None]
        else:
            raise ValueError(increments)
    spfh[counts == 0] = 0.0

    # ---- FPFH
    wsel = d2 != 0
    W = csr_matrix((1.0 / d2[wsel], (I[wsel], J[wsel])), shape=(n, n))
    acc = W @ spfh
    out = np.zeros((n, 33))
    for g in range(3):
        a = acc[:, 11 * g:11 * g + 11]
        s = a.sum(1)
        nz = s != 0
        out[nz, 11 * g:11 * g + 11] = a[nz] * (100.0 / s[nz])[:, None]
    out[~finite] = np.nan

    # ---- fragile rows
    own = q["own"]
    fragile = own.copy()
    link = (q["inside"] | q["near_r"]) & own[q["Jc"]]   # (a pair within RADIUS_TOL of r2 links its two rows whichever side it is on)
    fragile[q["Ic"][link]] = True
    fragile &= finite
    return out, spfh, m, fragile
