"""Reference of pcl::MovingLeastSquares::process with upsampling VOXEL_GRID_DILATION (PCL 1.7.x surface/impl/mls.hpp:
computeMLSPointNormal's MLSResult, MLSVoxelGrid, performUpsampling's VOXEL_GRID_DILATION branch, projectPointToMLSSurface), in numpy
float64 / float32 and in PCL's order of operations.  It reuses the pieces of mls_ref (eigen33, unit_orthogonal, llt_solve, seq_sum,
neighbourhoods, the cloud generators).  PCL is not on the machines, so this file is the pin.

Three stated deviations from PCL (include/ope.h): non-finite input points are dropped, are nobody's neighbour and nobody's nearest
point; a Cholesky pivot that is <= 0 or not finite makes the fit count as failed (the polynomial is not applied); a dilation
neighbour with a cell component outside [0, data_size) is dropped where PCL lets the unsigned key wrap.  Ties of the 1-nearest search
(equal fp32 distances) go to the lowest original index.
"""
import numpy as np

import mls_ref
from mls_ref import eigen33, llt_solve, nr_coeff, seq_sum, unit_orthogonal

F32 = np.float32
MAX_ORDER = 4
MAX_COEFF = nr_coeff(MAX_ORDER)


def mls_result(q, nb, order=2, polynomial_fit=True, sqr_gauss_param=1.0):
    """MLSResult of one query q (float32 xyz) with its neighbours nb ((m, 3) float32, m >= 3): dict(mean, n, u, v fp64 (3,); c fp64
    (nr_coeff,) or None; m; curvature float32; fit_failed).  mean: q projected on its plane, before any polynomial move."""
    P = np.asarray(nb, F32).astype(np.float64)
    q = np.asarray(q, F32).astype(np.float64)
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
    mean = q - dist * n
    curv = F32(cov[0, 0] + cov[1, 1] + cov[2, 2])
    if curv != 0:
        with np.errstate(all="ignore"):
            curv = F32(abs(F32(ev / np.float64(curv))))
    u, v, c, failed = np.zeros(3), np.zeros(3), None, False
    nc = nr_coeff(order)
    if polynomial_fit and m >= nc:
        v = unit_orthogonal(n)
        u = np.array([n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]])
        de = P - mean
        sq = ((de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]) + de[:, 2] * de[:, 2]).astype(F32)
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
        A = np.cumsum(PW[:, None, :] * Pm[None, :, :], axis=2)[:, :, -1]   # each entry summed in index order, as seq_sum does
        b = np.cumsum(PW * f[None, :], axis=1)[:, -1]
        c = llt_solve(A, b)
        if c is None:
            failed = True
    return dict(mean=mean, n=n, u=u, v=v, c=c, m=m, curvature=curv, fit_failed=failed)


def mls_results(xyz, radius, order=2, polynomial_fit=True, sqr_gauss_param=None, nbh=None):
    """MLSResult per ORIGINAL index as arrays: valid bool (n,), mean / n / u / v fp64 (n, 3), c fp64 (n, 15) (NaN where there is no
    solution), m int (n,) (0 for non-finite points), curvature float32 (n,), fit_failed bool (n,)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    sgp = float(radius) * float(radius) if not sqr_gauss_param else float(sqr_gauss_param)
    fin, offs, nidx, _ = nbh if nbh is not None else mls_ref.neighbourhoods(xyz, radius)
    N = len(xyz)
    r = dict(valid=np.zeros(N, bool), mean=np.zeros((N, 3)), n=np.zeros((N, 3)), u=np.zeros((N, 3)), v=np.zeros((N, 3)),
             c=np.full((N, MAX_COEFF), np.nan), m=np.zeros(N, np.int64), curvature=np.zeros(N, F32), fit_failed=np.zeros(N, bool))
    for k, i in enumerate(fin):
        nb = nidx[offs[k]:offs[k + 1]]
        r["m"][i] = len(nb)
        if len(nb) < 3:
            continue
        one = mls_result(xyz[i], xyz[nb], order, polynomial_fit, sgp)
        r["valid"][i] = True
        for key in ("mean", "n", "u", "v"):
            r[key][i] = one[key]
        if one["c"] is not None:
            r["c"][i, :len(one["c"])] = one["c"]
        r["curvature"][i] = one["curvature"]
        r["fit_failed"][i] = one["fit_failed"]
    return r


# --------------------------------------------------------------------------------------------------------------- MLSVoxelGrid
def voxel_box(xyz):
    fin = np.isfinite(xyz).all(axis=1)
    return xyz[fin].min(axis=0).astype(F32), xyz[fin].max(axis=0).astype(F32)


def data_size_of(bmin, bmax, voxel_size):
    ext = float((bmax - bmin).max())   # float subtraction, then widened
    return int(1.5 * ext / float(F32(voxel_size)))


def decode_keys(keys, data_size):
    """getIndexIn3D: (cell0, cell1, cell2) of 1-D keys; data_size 0 (every point within 2/3 of a voxel) decodes to cell (0, 0, 0)."""
    keys = np.asarray(keys, np.int64)
    if data_size == 0:
        return np.zeros((len(keys), 3), np.int64)
    c0, rem = np.divmod(keys, data_size * data_size)
    c1, c2 = np.divmod(rem, data_size)
    return np.stack([c0, c1, c2], axis=1)


def voxel_keys(xyz, voxel_size, dilation_iterations=0):
    """The grid: (ascending distinct keys int64, data_size, bmin float32 (3,)).  Empty when no point is finite."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return np.zeros(0, np.int64), 0, np.zeros(3, F32)
    vs = F32(voxel_size)
    bmin, bmax = voxel_box(xyz)
    ds = data_size_of(bmin, bmax, vs)
    cell = ((xyz[fin] - bmin) / vs).astype(np.int32).astype(np.int64)   # float subtract, float divide, truncate
    keys = set(((cell[:, 0] * ds + cell[:, 1]) * ds + cell[:, 2]).tolist())
    for _ in range(dilation_iterations):
        new = set()
        for key in keys:
            if ds == 0:
                continue
            c0, rem = divmod(key, ds * ds)
            c1, c2 = divmod(rem, ds)
            for x in (-1, 0, 1):
                for y in (-1, 0, 1):
                    for z in (-1, 0, 1):
                        a, b, c = c0 + x, c1 + y, c2 + z
                        if 0 <= a < ds and 0 <= b < ds and 0 <= c < ds:   # the deviation: PCL lets the unsigned key wrap
                            new.add((a * ds + b) * ds + c)
        keys = new
    return np.array(sorted(keys), np.int64), ds, bmin


def voxel_positions(keys, data_size, bmin, voxel_size):
    """float(cell) * voxel_size + bmin: a float multiply, then a float add."""
    cell = decode_keys(keys, data_size).astype(F32)
    return (cell * F32(voxel_size)).astype(F32) + bmin.astype(F32)


def nearest_lowest_index(pos, xyz, chunk=2048):
    """k = 1 among the finite points in fp32 (dx^2 + dy^2) + dz^2; exact ties go to the lowest original index."""
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    P = xyz[fin].astype(F32)
    out = np.empty(len(pos), np.int64)
    for s in range(0, len(pos), chunk):
        d = pos[s:s + chunk, None, :].astype(F32) - P[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        out[s:s + chunk] = fin[np.argmin(d2, axis=1)]   # argmin: the first minimum, and `fin` ascends
    return out


def dot3_f32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]   # float32 arrays: unfused float operations


def norm3_f32(a):
    return np.sqrt(dot3_f32(a, a))


def project(res, j, u_disp, v_disp, order, polynomial_fit):
    """projectPointToMLSSurface for voxels whose nearest points are j ((k,) original indices, all valid), vectorised over the voxels.
    Returns (result fp64 (k, 3) before the cast, normal fp64 (k, 3), applied bool (k,), n_disp fp64 (k,))."""
    nc = nr_coeff(order)
    c = res["c"][j]
    with np.errstate(invalid="ignore"):
        applied = np.full(len(j), bool(polynomial_fit)) & (res["m"][j] >= 5 * nc) & np.isfinite(c[:, 0]) & ~res["fit_failed"][j]
    n_disp, d_u, d_v = np.zeros(len(j)), np.zeros(len(j)), np.zeros(len(j))
    ca = np.where(applied[:, None], np.nan_to_num(c), 0.0)
    k = 0
    u_pow, u_pow_prev = np.ones(len(j), F32), np.ones(len(j), F32)
    for ui in range(order + 1):
        v_pow, v_pow_prev = np.ones(len(j), F32), np.ones(len(j), F32)
        for vi in range(order - ui + 1):
            n_disp = n_disp + (u_pow * v_pow).astype(np.float64) * ca[:, k]
            if ui >= 1:
                d_u = d_u + ca[:, k] * (float(ui) * (u_pow_prev * v_pow).astype(np.float64))
            if vi >= 1:
                d_v = d_v + ca[:, k] * (float(vi) * (u_pow * v_pow_prev).astype(np.float64))
            k += 1
            v_pow_prev = v_pow
            v_pow = v_pow * v_disp
        u_pow_prev = u_pow
        u_pow = u_pow * u_disp
    n_disp, d_u, d_v = (np.where(applied, x, 0.0) for x in (n_disp, d_u, d_v))
    mean, n, u, v = res["mean"][j], res["n"][j], res["u"][j], res["v"][j]
    ud, vd = u_disp.astype(np.float64)[:, None], v_disp.astype(np.float64)[:, None]
    result = ((mean + u * ud) + v * vd) + n * n_disp[:, None]
    nrm = (n - d_u[:, None] * u) - d_v[:, None] * v
    nrm = nrm / np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])[:, None]
    return result, nrm, applied, n_disp


def mls_upsample(xyz, radius, order=2, polynomial_fit=True, compute_normals=False, sqr_gauss_param=None, voxel_size=1.0,
                 dilation_iterations=0, nbh=None, results=None):
    """The operator over a cloud.  Returns dict(xyz float32 (k, 3), normals float32 (k, 3) (the plane's normal of point idx unless
    compute_normals), curvature float32 (k,), idx int32 (k,), stats dict, and per VOXEL in key order: keys, pos, nearest, near_valid, keep,
    d_before, d_after, result float32, normal float32, curvature_vox (that of the nearest point), applied, n_disp)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    res = results if results is not None else mls_results(xyz, radius, order, polynomial_fit, sqr_gauss_param, nbh)
    keys, ds, bmin = voxel_keys(xyz, voxel_size, dilation_iterations)
    nv = len(keys)
    stats = dict(n_in=len(xyz), n_valid=int(res["valid"].sum()), n_voxels=nv, n_invalid_nearest=0, n_polynomial=0, n_rejected_farther=0,
                 n_out=0, data_size=ds)
    empty = dict(xyz=np.zeros((0, 3), F32), normals=np.zeros((0, 3), F32), curvature=np.zeros(0, F32), idx=np.zeros(0, np.int32),
                 stats=stats, keys=keys)
    if nv == 0:
        return empty
    pos = voxel_positions(keys, ds, bmin, voxel_size)
    near = nearest_lowest_index(pos, xyz)
    ok = res["valid"][near]
    stats["n_invalid_nearest"] = int((~ok).sum())
    jv = near[ok]
    qj = xyz[jv]
    dd = pos[ok] - qj
    u_disp = dot3_f32(dd, res["u"][jv].astype(F32))
    v_disp = dot3_f32(dd, res["v"][jv].astype(F32))
    r64, nrm64, applied, n_disp = project(res, jv, u_disp, v_disp, order, polynomial_fit)
    r32 = r64.astype(F32)
    d_before = norm3_f32(dd)
    d_after = norm3_f32(r32 - qj)
    keep_ok = ~(d_after > d_before)
    stats["n_polynomial"] = int(applied.sum())
    stats["n_rejected_farther"] = int((~keep_ok).sum())
    stats["n_out"] = int(keep_ok.sum())

    def per_voxel(a, fill=0):
        out = np.full((nv,) + a.shape[1:], fill, a.dtype)
        out[ok] = a
        return out

    keep = per_voxel(keep_ok, False)
    normal = nrm64.astype(F32) if compute_normals else res["n"][jv].astype(F32)
    sel = keep_ok
    return dict(xyz=r32[sel], normals=normal[sel], curvature=res["curvature"][jv][sel], idx=jv[sel].astype(np.int32), stats=stats,
                keys=keys, pos=pos, nearest=near, near_valid=ok, keep=keep, d_before=per_voxel(d_before), d_after=per_voxel(d_after),
                result=per_voxel(r32), normal=per_voxel(normal), curvature_vox=res["curvature"][near], applied=per_voxel(applied, False), n_disp=per_voxel(n_disp))


# ---------------------------------------------------------------------------------------------------------------- test clouds
RADIUS = 0.03
ORDER = 4
VOXEL = 0.002
SEED = 3


def upsample_cloud(seed=SEED):
    """The GPU test's cloud: mls_ref.base_cloud without its 2 500-point clump.  Two surfaces of 1 500 points each, then isolated
    points, pairs, triples, quintuples, 10 exact duplicates and 7 non-finite points.  Returns (xyz float32, n_surface)."""
    rng = np.random.default_rng(seed)
    surf = np.r_[mls_ref.paraboloid_patch(rng, 1500), mls_ref.sphere_points(rng, 1500, max_polar=np.radians(75.0))]
    parts = [surf]
    far = lambda k: np.array([-0.5 + 0.1 * k, 0.6, 0.9])
    parts.append(np.array([far(k) for k in range(5)]))
    for k in (5, 6):
        parts.append(far(k) + rng.uniform(-0.003, 0.003, (2, 3)))
    for k, m in ((7, 3), (8, 3), (9, 3), (10, 5), (11, 5)):
        parts.append(far(k) + rng.uniform(-0.003, 0.003, (m, 3)))
    parts.append(surf[rng.choice(len(surf), 10, replace=False)])
    xyz = np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(F32)
    bad_at = np.sort(rng.choice(len(xyz), 7, replace=False))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [1, np.nan, 1], [np.inf, np.inf, 1], [0.9, 0.9, np.nan]], F32)
    for k, at in enumerate(bad_at):
        xyz = np.insert(xyz, at + k, bad[k], axis=0)
    return np.ascontiguousarray(xyz, F32), len(surf)


def undecided(ref, ulps=8):
    """Voxels (bool per voxel) whose keep decision hangs on at most `ulps` float ulps of d_before: the device may keep or drop them."""
    gap = np.abs(ref["d_before"].astype(np.float64) - ref["d_after"].astype(np.float64))
    return ref["near_valid"] & (gap <= ulps * np.spacing(ref["d_before"]).astype(np.float64))
