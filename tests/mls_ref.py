"""Reference of pcl::MovingLeastSquares::process with upsampling NONE (PCL 1.7.x surface/impl/mls.hpp, computeMLSPointNormal),
step by step in numpy float64 and in PCL's order of operations: compute3DCentroid, computeCovarianceMatrix (unnormalised), pcl::eigen33
with computeRoots in double, the plane, the projected query, Eigen's unitOrthogonal, the polynomial's terms in PCL's order, the
weighted normal equations and Eigen's unblocked lower Cholesky (LLT::solveInPlace).  Neighbourhoods come from oracle.KdTree's radius
search over the finite points (ascending distance, the order PCL's sorted radius search hands them over in).

Two stated deviations from PCL (include/ope.h): non-finite input points are dropped and are nobody's neighbour; a Cholesky pivot
that is <= 0 or not finite makes the fit fail like a non-finite c[0].
"""
import math

import numpy as np

import oracle

EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny


def nr_coeff(order):
    return (order + 1) * (order + 2) // 2


def seq_sum(a):
    """Sum along axis 0 in index order, one addition after the other as a C++ loop adds (numpy's own sum adds pairwise)."""
    return np.cumsum(a, axis=0)[-1]


def compute_roots2(b, c):
    d = b * b - 4.0 * c
    if d < 0.0:
        d = 0.0
    sd = math.sqrt(d)
    return [0.0, 0.5 * (b - sd), 0.5 * (b + sd)]


def compute_roots(m):
    """pcl::computeRoots (common/impl/eigen.hpp), Scalar = double; m: 3x3 symmetric."""
    c0 = (m[0][0] * m[1][1] * m[2][2] + 2.0 * m[0][1] * m[0][2] * m[1][2] - m[0][0] * m[1][2] * m[1][2]
          - m[1][1] * m[0][2] * m[0][2] - m[2][2] * m[0][1] * m[0][1])
    c1 = m[0][0] * m[1][1] - m[0][1] * m[0][1] + m[0][0] * m[2][2] - m[0][2] * m[0][2] + m[1][1] * m[2][2] - m[1][2] * m[1][2]
    c2 = m[0][0] + m[1][1] + m[2][2]
    if abs(c0) < EPS:
        return compute_roots2(c2, c1)
    s_inv3 = 1.0 / 3.0
    s_sqrt3 = math.sqrt(3.0)
    c2_over_3 = c2 * s_inv3
    a_over_3 = (c1 - c2 * c2_over_3) * s_inv3
    if a_over_3 > 0.0:
        a_over_3 = 0.0
    half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1))
    q = half_b * half_b + a_over_3 * a_over_3 * a_over_3
    if q > 0.0:
        q = 0.0
    rho = math.sqrt(-a_over_3)
    theta = math.atan2(math.sqrt(-q), half_b) * s_inv3
    cos_theta, sin_theta = math.cos(theta), math.sin(theta)
    r = [c2_over_3 + 2.0 * rho * cos_theta,
         c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta),
         c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta)]
    if r[0] >= r[1]:
        r[0], r[1] = r[1], r[0]
    if r[1] >= r[2]:
        r[1], r[2] = r[2], r[1]
        if r[0] >= r[1]:
            r[0], r[1] = r[1], r[0]
    if r[0] <= 0.0:
        return compute_roots2(c2, c1)
    return r


def eigen33(mat):
    """pcl::eigen33 (mat, eigenvalue, eigenvector): the smallest eigenpair of a symmetric 3x3 matrix."""
    mat = np.asarray(mat, np.float64)
    scale = float(np.max(np.abs(mat)))
    if scale <= TINY:
        scale = 1.0
    sm = (mat / scale).tolist()
    roots = compute_roots(sm)
    eigenvalue = roots[0] * scale
    for d in range(3):
        sm[d][d] -= roots[0]
    r0, r1, r2 = sm

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    v1, v2, v3 = cross(r0, r1), cross(r0, r2), cross(r1, r2)
    l1, l2, l3 = (sum(x * x for x in v) for v in (v1, v2, v3))   # (x*x + y*y) + z*z
    if l1 >= l2 and l1 >= l3:
        v, ln = v1, l1
    elif l2 >= l1 and l2 >= l3:
        v, ln = v2, l2
    else:
        v, ln = v3, l3
    with np.errstate(all="ignore"):
        vec = np.array(v, np.float64) / np.sqrt(np.float64(ln))
    return eigenvalue, vec


def unit_orthogonal(n):
    """Eigen's unitOrthogonal for 3-vectors (Geometry/OrthoMethods.h)."""
    x, y, z = float(n[0]), float(n[1]), float(n[2])
    if abs(x) > abs(z) * 1e-12 or abs(y) > abs(z) * 1e-12:
        invnm = 1.0 / math.sqrt(x * x + y * y)
        return np.array([-y * invnm, x * invnm, 0.0])
    invnm = 1.0 / math.sqrt(y * y + z * z)
    return np.array([0.0, -z * invnm, y * invnm])


def llt_solve(A, b):
    """Eigen::LLT (llt_inplace<Lower>::unblocked) and solveInPlace; None when a pivot is <= 0 or not finite."""
    A = np.array(A, np.float64)
    n = len(A)
    for k in range(n):
        x = A[k, k]
        if k > 0:
            x = x - sum(A[k, j] * A[k, j] for j in range(k))
        if not (x > 0.0) or not math.isfinite(x):
            return None
        x = math.sqrt(x)
        A[k, k] = x
        rx = 1.0 / x
        for i in range(k + 1, n):
            if k > 0:
                A[i, k] -= sum(A[i, j] * A[k, j] for j in range(k))
            A[i, k] *= rx
    c = np.array(b, np.float64)
    for i in range(n):
        t = c[i]
        for j in range(i):
            t -= A[i, j] * c[j]
        c[i] = t / A[i, i]
    for i in range(n - 1, -1, -1):
        t = c[i]
        for j in range(i + 1, n):
            t -= A[j, i] * c[j]
        c[i] = t / A[i, i]
    return c


def mls_point(q, nb, order=2, polynomial_fit=True, sqr_gauss_param=1.0):
    """One query q (float32 xyz) with its neighbours nb ((m, 3) float32, m >= 3): (point fp64, normal fp64, curvature float32, fitted, the plane's normal fp64)."""
    P = np.asarray(nb, np.float32).astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64)
    m = len(P)
    centroid = seq_sum(P) / m
    d = P - centroid
    cov = np.zeros((3, 3))
    cov[1, 1], cov[1, 2], cov[2, 2] = seq_sum(d[:, 1] * d[:, 1]), seq_sum(d[:, 1] * d[:, 2]), seq_sum(d[:, 2] * d[:, 2])
    dx = d * d[:, :1]
    cov[0, 0], cov[0, 1], cov[0, 2] = seq_sum(dx[:, 0]), seq_sum(dx[:, 1]), seq_sum(dx[:, 2])
    cov[1, 0], cov[2, 0], cov[2, 1] = cov[0, 1], cov[0, 2], cov[1, 2]
    ev, n = eigen33(cov)
    d4 = -1.0 * (n[0] * centroid[0] + n[1] * centroid[1] + n[2] * centroid[2])
    dist = (q[0] * n[0] + q[1] * n[1] + q[2] * n[2]) + d4
    point = q - dist * n
    curv = np.float32(cov[0, 0] + cov[1, 1] + cov[2, 2])
    if curv != 0:
        with np.errstate(all="ignore"):
            curv = np.float32(abs(np.float32(ev / np.float64(curv))))
    normal = n.copy()
    fitted = False
    nc = nr_coeff(order)
    if polynomial_fit and m >= nc:
        v = unit_orthogonal(n)
        u = np.array([n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]])
        de = P - point
        sq = ((de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]) + de[:, 2] * de[:, 2]).astype(np.float32)
        w = np.exp((-sq).astype(np.float64) / sqr_gauss_param)
        uc = (de[:, 0] * u[0] + de[:, 1] * u[1]) + de[:, 2] * u[2]
        vc = (de[:, 0] * v[0] + de[:, 1] * v[1]) + de[:, 2] * v[2]
        f = (de[:, 0] * n[0] + de[:, 1] * n[1]) + de[:, 2] * n[2]
        Pm = np.zeros((nc, m))
        j = 0
        u_pow = np.ones(m)
        for ui in range(order + 1):
            v_pow = np.ones(m)
            for vi in range(order - ui + 1):
                Pm[j] = u_pow * v_pow
                j += 1
                v_pow = v_pow * vc
            u_pow = u_pow * uc
        PW = Pm * w[None, :]
        A = np.zeros((nc, nc))
        b = np.zeros(nc)
        for i in range(nc):
            for j in range(nc):
                A[i, j] = seq_sum(PW[i] * Pm[j])
            b[i] = seq_sum(PW[i] * f)
        c = llt_solve(A, b)
        if c is not None and math.isfinite(c[0]):
            fitted = True
            point = point + c[0] * n
            if order >= 1:
                normal = (n - c[order + 1] * u) - c[1] * v
    return point, normal, curv, fitted, n


def neighbourhoods(xyz, radius):
    """Radius neighbourhoods of the finite points among the finite points (oracle.KdTree): (finite idx, offsets, neighbour idx (original), d2)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1)).astype(np.int32)
    if len(fin) == 0:
        return fin, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    tree = oracle.KdTree(xyz[fin])
    offs, idx, d2 = tree.radius(xyz[fin], float(radius), True)
    return fin, offs, fin[idx], d2


def mls_smooth(xyz, radius, order=2, polynomial_fit=True, compute_normals=False, sqr_gauss_param=None, nbh=None):
    """The operator over a cloud.  Returns dict(xyz float32 (m, 3), normals float32 (m, 3), curvature float32 (m,), idx int32 (m,),
    stats dict, xyz64 the positions before the cast).  normals are the plane's normal unless compute_normals."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    sgp = float(radius) * float(radius) if not sqr_gauss_param else float(sqr_gauss_param)
    fin, offs, nidx, _ = nbh if nbh is not None else neighbourhoods(xyz, radius)
    out_p, out_n, out_c, out_i = [], [], [], []
    plane_only = 0
    for k, i in enumerate(fin):
        nb = nidx[offs[k]:offs[k + 1]]
        if len(nb) < 3:
            continue
        point, normal, curv, fitted, plane_normal = mls_point(xyz[i], xyz[nb], order, polynomial_fit, sgp)
        if not fitted:
            plane_only += 1
        if not compute_normals:
            normal = plane_normal
        out_p.append(point); out_n.append(normal); out_c.append(curv); out_i.append(i)
    m = len(out_i)
    p64 = np.array(out_p, np.float64).reshape(m, 3)
    stats = dict(n_in=len(xyz), n_out=m, n_plane_only=plane_only, n_dropped=len(xyz) - m, neighbours_total=int(offs[-1]))
    return dict(xyz=p64.astype(np.float32), xyz64=p64, normals=np.array(out_n, np.float64).reshape(m, 3).astype(np.float32),
                curvature=np.array(out_c, np.float32).reshape(m), idx=np.array(out_i, np.int32).reshape(m), stats=stats)


# ---------------------------------------------------------------------------------------------------------------- test clouds
RADIUS = 0.02
BASE_SEED = 3


def paraboloid_patch(rng, n, side=0.22, centre=(0.0, 0.0, 1.0), noise=0.0005):
    """Jittered points on z = 2 (x^2 + y^2) about `centre`, plus isotropic noise."""
    uv = rng.uniform(-side / 2, side / 2, (n, 2))
    p = np.c_[uv, 2.0 * (uv ** 2).sum(axis=1)] + np.asarray(centre)
    return (p + rng.normal(0.0, noise, p.shape)).astype(np.float32)


def sphere_points(rng, n, R=0.1, centre=(0.4, 0.0, 1.0), noise=0.0005, max_polar=np.pi):
    """Uniform points on a sphere (or the cap within max_polar of +z), displaced radially by N(0, noise)."""
    z = rng.uniform(np.cos(max_polar), 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - z * z)
    d = np.c_[s * np.cos(phi), s * np.sin(phi), z]
    r = R + rng.normal(0.0, noise, n)
    return (d * r[:, None] + np.asarray(centre)).astype(np.float32)


def radial_rms(xyz, R=0.1, centre=(0.4, 0.0, 1.0)):
    d = np.linalg.norm(np.asarray(xyz, np.float64) - np.asarray(centre), axis=1) - R
    return float(np.sqrt(np.mean(d * d)))


def base_cloud(seed=BASE_SEED):
    """The GPU test's cloud: ~3 k surface points with 10-80 neighbours, then the special cases.  Returns (xyz float32, info)."""
    rng = np.random.default_rng(seed)
    surf = np.r_[paraboloid_patch(rng, 1500), sphere_points(rng, 1500, max_polar=np.radians(75.0))]
    parts = [surf]
    far = lambda k: np.array([-0.5 + 0.1 * k, 0.6, 0.9])   # spots 10 cm apart, far from both surfaces
    parts.append(np.array([far(k) for k in range(5)]))                                            # 5 isolated points
    for k in (5, 6):                                                                               # two pairs
        parts.append(far(k) + rng.uniform(-0.003, 0.003, (2, 3)))
    for k, m in ((7, 3), (8, 3), (9, 3), (10, 5), (11, 5)):                                         # triples and quintuples
        parts.append(far(k) + rng.uniform(-0.003, 0.003, (m, 3)))
    parts.append(surf[rng.choice(len(surf), 10, replace=False)])                                   # 10 exact duplicates
    d = rng.normal(size=(2500, 3))
    d *= (0.005 * rng.uniform(0, 1, 2500) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
    parts.append(np.array([0.0, -0.6, 1.0]) + d)                                                   # 2 500 points in a ball of 1 cm
    xyz = np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(np.float32)
    bad_at = np.sort(rng.choice(len(xyz), 7, replace=False))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [1, np.nan, 1], [np.inf, np.inf, 1], [0.9, 0.9, np.nan]],
                   np.float32)
    for k, at in enumerate(bad_at):
        xyz = np.insert(xyz, at + k, bad[k], axis=0)                                               # 7 non-finite points
    return np.ascontiguousarray(xyz, np.float32), dict(n_surface=len(surf))


def pairs_near_radius(xyz, radius, ulps=4):
    """Pairs whose float d2 lies within `ulps` float ulps of float(radius)^2, from the oracle's own d2."""
    r2 = np.float32(radius) * np.float32(radius)
    _, _, _, d2 = neighbourhoods(xyz, float(radius) * 1.01)
    return int(np.count_nonzero(np.abs(d2.astype(np.float64) - np.float64(r2)) <= ulps * np.float64(np.spacing(r2))))
