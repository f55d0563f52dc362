"""Deterministic synthetic clouds for the BASELINE.json configs.

model  = points on a closed, asymmetric star-shaped surface inside a 0.2 m box
         (superellipsoid radial function + 3 Gaussian bumps), area-weighted
         rejection sampling, fp32.
scene  = the same surface re-sampled independently (different sample points, so
         NN distances are non-zero) + 10 % uniform clutter in a 0.4 m box, moved
         by the ground-truth pose Rz(12°)·Ry(−7°)·Rx(5°), t=(0.015,−0.010,0.020) m,
         plus N(0,(0.5 mm)²) noise, then shuffled (sensor order is not spatial).

numpy's PCG64 stream is platform-independent, so both boxes generate identical
clouds from the seeds alone; nothing is read from disk.
"""
from __future__ import annotations

import numpy as np

# Round 1's body (axes 0.100/0.075/0.050, bumps of +22 %, -15 %, +30 %) was nearly symmetric under the half turns
# about its axes: ICP had a stable minimum at each of them whose residual was within 1 % of the true one, and
# SAC-IA could not tell them apart.  The bumps are now features of the size of the body itself — a
# grip-like lobe, a nose and a dent, like the reference's drill — so no half turn maps the surface near itself.
_AXES = np.array([0.080, 0.050, 0.040])          # superellipsoid semi-axes (m)
_POW = 2.5
_BUMP_DIR = np.array([[0.85, 0.40, 0.30], [-0.45, 0.85, -0.25], [0.15, -0.50, 0.85]])
_BUMP_DIR = _BUMP_DIR / np.linalg.norm(_BUMP_DIR, axis=1, keepdims=True)
_BUMP_AMP = np.array([0.45, 0.95, -0.35])
_BUMP_SIG = np.array([0.32, 0.30, 0.45])          # radians


def _radius(u: np.ndarray) -> np.ndarray:
    """Radial function r(u) of the star-shaped model surface; u unit vectors (n,3)."""
    se = (np.abs(u / _AXES) ** _POW).sum(axis=1) ** (-1.0 / _POW)
    ang = np.arccos(np.clip(u @ _BUMP_DIR.T, -1.0, 1.0))           # (n,3)
    bump = (_BUMP_AMP * np.exp(-(ang / _BUMP_SIG) ** 2)).sum(axis=1)
    return se * (1.0 + bump)


def _sample_dirs(rng: np.random.Generator, m: int) -> np.ndarray:
    v = rng.standard_normal((m, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def model_surface(n: int, seed: int = 1, return_normals: bool = False):
    """n points on the model surface, approximately area-uniform. float32 (n,3)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 3), np.float64)
    nrm = np.empty((n, 3), np.float64) if return_normals else None
    got = 0
    h = 1e-4
    w_max = None
    while got < n:
        m = max(4096, int((n - got) * 2.2))
        u = _sample_dirs(rng, m)
        # tangent frame
        a = np.where(np.abs(u[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
        e1 = np.cross(u, a); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = np.cross(u, e1)
        r = _radius(u)

        def rr(d):
            q = u + h * d
            return _radius(q / np.linalg.norm(q, axis=1, keepdims=True))

        g1 = (rr(e1) - rr(-e1)) / (2 * h)
        g2 = (rr(e2) - rr(-e2)) / (2 * h)
        w = r * np.sqrt(r * r + g1 * g1 + g2 * g2)          # dA/dΩ
        if w_max is None:
            w_max = 1.25 * w.max()
        keep = rng.random(m) * w_max < w
        p = (u * r[:, None])[keep]
        k = min(len(p), n - got)
        out[got:got + k] = p[:k]
        if return_normals:
            # surface normal of p(u)=r(u)u :  n ∝ r u − ∇_S r
            nn = (r[:, None] * u - g1[:, None] * e1 - g2[:, None] * e2)[keep][:k]
            nrm[got:got + k] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
        got += k
    if return_normals:
        return out.astype(np.float32), nrm.astype(np.float32)
    return out.astype(np.float32)


def rot_xyz(rx_deg: float, ry_deg: float, rz_deg: float) -> np.ndarray:
    """Rz·Ry·Rx (degrees) as float64 (3,3)."""
    rx, ry, rz = np.deg2rad([rx_deg, ry_deg, rz_deg])
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


GT_R = rot_xyz(5.0, -7.0, 12.0)
GT_T = np.array([0.015, -0.010, 0.020])


def workspace_limits(margin: float = 0.01):
    """(lo, hi) of the pass-through crop the reference applies to a captured frame before anything else
    (`ProcessingPcd::getPassThrough` with the `-l` limits, rosinterface.cpp:212): here the box an operator would set
    around the object — the posed model's bounding box plus `margin` (m)."""
    m = model_surface(20_000, 1).astype(np.float64) @ GT_R.T + GT_T
    return (m.min(0) - margin).astype(np.float32), (m.max(0) + margin).astype(np.float32)


def ground_truth_pose() -> np.ndarray:
    """4x4 (math layout) that maps model coordinates to scene coordinates."""
    T = np.eye(4)
    T[:3, :3] = GT_R
    T[:3, 3] = GT_T
    return T


def scene_cloud(n: int, seed_surface: int = 2, seed_clutter: int = 3, seed_noise: int = 4,
                clutter_frac: float = 0.10, noise_sigma: float = 0.0005, shuffle: bool = True,
                R: np.ndarray | None = None, t: np.ndarray | None = None) -> np.ndarray:
    """n scene points: re-sampled surface ∪ clutter, posed, noised. float32 (n,3)."""
    R = GT_R if R is None else R
    t = GT_T if t is None else t
    n_surf = int(round(n / (1.0 + clutter_frac)))
    n_clut = n - n_surf
    surf = model_surface(n_surf, seed_surface).astype(np.float64)
    rc = np.random.default_rng(seed_clutter)
    clut = rc.uniform(-0.2, 0.2, size=(n_clut, 3))
    pts = np.concatenate([surf, clut], axis=0)
    pts = pts @ R.T + t
    rn = np.random.default_rng(seed_noise)
    pts += rn.standard_normal(pts.shape) * noise_sigma
    if shuffle:
        pts = pts[rn.permutation(len(pts))]
    return pts.astype(np.float32)


def config_clouds(name: str):
    """(scene=source, model=target) for a BASELINE.json config: 'C2' or 'C3'."""
    if name == "C2":
        return scene_cloud(100_000), model_surface(20_000, 1)
    if name == "C3":
        return scene_cloud(1_000_000), model_surface(100_000, 1)
    raise ValueError(name)


def bumpy_torus(n: int, seed: int = 11) -> np.ndarray:
    """KAT-1 cloud: points on a bumpy torus (unique ICP optimum). float32 (n,3)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, n)
    b = rng.uniform(0, 2 * np.pi, n)
    R0, r0 = 0.08, 0.03 * (1 + 0.3 * np.sin(3 * a) * np.cos(2 * b) + 0.2 * np.cos(a))
    x = (R0 + r0 * np.cos(b)) * np.cos(a)
    y = (R0 + r0 * np.cos(b)) * np.sin(a) * 0.8
    z = r0 * np.sin(b) + 0.01 * np.sin(2 * a)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def _frame_view(i: int, n_per_frame: int, noise_sigma: float, n_azimuths: int):
    az = 2.0 * np.pi * i / n_azimuths
    view = np.array([np.cos(az), np.sin(az), 0.35])
    view /= np.linalg.norm(view)
    pts = np.empty((0, 3))
    seed = 200 + i
    draw = 0
    while len(pts) < n_per_frame:
        p, nr = model_surface(int(n_per_frame * 2.4) + 1024, seed + 1000 * draw, return_normals=True)
        vis = p[(nr.astype(np.float64) @ view) > 0.05].astype(np.float64)
        pts = np.concatenate([pts, vis], axis=0)
        draw += 1
    pts = pts[:n_per_frame]
    rp = np.random.default_rng(100 + i)
    ang = rp.uniform(-3.0, 3.0, 3)
    T = np.eye(4)
    T[:3, :3] = rot_xyz(*ang)
    T[:3, 3] = rp.uniform(-0.005, 0.005, 3)
    pts = pts @ T[:3, :3].T + T[:3, 3]
    pts += np.random.default_rng(300 + i).standard_normal(pts.shape) * noise_sigma
    return pts.astype(np.float32), T


def frame_views(n_frames: int, n_per_frame: int, noise_sigma: float = 0.0002, return_poses: bool = False,
                n_azimuths: int | None = None, workers: int = 1):
    """BuildModel input (config C5): the model surface seen from `n_frames` azimuths.

    Frame i holds `n_per_frame` independently sampled surface points (seed 200+i) whose outward normal faces a
    viewer on the circle at azimuth 2πi/n_frames (back-face culled), moved by the frame's own small pose
    (≤3°, ≤5 mm, seed 100+i) and noised.  Returns a list of float32 (n_per_frame,3) arrays
    (+ the list of 4x4 frame poses if asked).  `n_azimuths` keeps C5's 32-step spacing with fewer frames.
    `workers` > 1: the frames are made by that many spawned processes (each frame has its own seeds: same arrays).
    """
    n_azimuths = n_frames if n_azimuths is None else n_azimuths
    args = [(i, n_per_frame, noise_sigma, n_azimuths) for i in range(n_frames)]
    out = None
    if workers > 1 and n_frames > 1:
        # child INTERPRETERS, not multiprocessing: a spawned multiprocessing worker imports the caller's __main__ again, and a
        # script without a __main__ guard then runs its whole body (its own frame_views call included) in every worker
        import os, subprocess, sys, tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        code = ("import importlib, sys, numpy as np; sys.path.insert(0, sys.argv[1]); "
                "s = importlib.import_module('object-pose-estimation_amd.synth'); "
                "f, T = s._frame_view(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5])); "
                "np.save(sys.argv[6] + '.f.npy', f); np.save(sys.argv[6] + '.T.npy', T)")
        try:
            with tempfile.TemporaryDirectory() as tmp:
                out = [None] * n_frames
                pending = list(range(n_frames))
                running = []
                while pending or running:
                    while pending and len(running) < workers:
                        i = pending.pop(0)
                        base = os.path.join(tmp, f"frame{i}")
                        running.append((i, base, subprocess.Popen([sys.executable, "-c", code, root, str(i), str(n_per_frame), repr(float(noise_sigma)),
                                                                   str(n_azimuths), base], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
                    i, base, pr = running.pop(0)
                    if pr.wait(timeout=1800) != 0:
                        raise RuntimeError("frame worker failed")
                    out[i] = (np.load(base + ".f.npy"), np.load(base + ".T.npy"))
        except Exception:
            out = None
    if out is None:
        out = [_frame_view(*a) for a in args]
    frames, poses = [f for f, _ in out], [T for _, T in out]
    return (frames, poses) if return_poses else frames


def _box_surface(rng: np.random.Generator, size, n: int) -> np.ndarray:
    """n points on the surface of an axis-aligned box of edge lengths `size`, centred at 0, area-uniform."""
    sx, sy, sz = size
    faces = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    f = rng.choice(6, n, p=faces / faces.sum())
    u = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(size)
    ax, sign = f // 2, np.where(f % 2 == 0, -0.5, 0.5)
    u[np.arange(n), ax] = sign * np.array(size)[ax]
    return u


def _cylinder_surface(rng: np.random.Generator, r: float, h: float, n: int) -> np.ndarray:
    """n points on the mantle and the top disc of an upright cylinder (axis z, base at z = -h/2)."""
    a_side, a_top = 2 * np.pi * r * h, np.pi * r * r
    top = rng.random(n) < a_top / (a_side + a_top)
    phi = rng.uniform(0, 2 * np.pi, n)
    rad = np.where(top, r * np.sqrt(rng.random(n)), r)
    z = np.where(top, h / 2, rng.uniform(-h / 2, h / 2, n))
    return np.stack([rad * np.cos(phi), rad * np.sin(phi), z], axis=1)


def _sphere_cap(rng: np.random.Generator, r: float, n: int) -> np.ndarray:
    """n points on the upper half of a sphere of radius r (the half a camera above the table sees)."""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 2] = np.abs(v[:, 2])
    return r * v


def tabletop_objects(n_drill: int = 8000, density: float = 62500.0, seed: int = 21):
    """The non-plane cloud of one table-top frame (what ObjectSegmentationPlane hands to getClusters): the model ("drill")
    surface at the ground-truth pose, four distractors at camera-like density (`density` points per m^2: 4 mm spacing by
    default) standing on a table 0.12 m below the model's centre (two boxes, a cylinder, a sphere cap), five stray blobs of
    40-250 points and a thin strip of table edge, shuffled.  The cylinder stands 3 cm from the first box, under the reference's
    5 cm tolerance, so the two are one cluster; every other gap is at least 10 cm.
    Returns (points float32 (n, 3), object id int32 (n,)): 0 the model, 1 box, 2 cylinder (merges with 1), 3 sphere cap,
    4 second box, 5 table-edge strip, 6-10 the blobs."""
    rng = np.random.default_rng(seed)
    parts, ids = [], []

    def add(p, i):
        parts.append(np.asarray(p, np.float64))
        ids.append(np.full(len(p), i, np.int32))

    add(model_surface(n_drill, seed + 1).astype(np.float64) @ GT_R.T + GT_T, 0)
    table_z = GT_T[2] - 0.12
    box = (0.08, 0.06, 0.10)
    box_c = np.array([0.40, 0.0, table_z + box[2] / 2])
    add(_box_surface(rng, box, int(density * 2 * (box[0] * box[1] + box[0] * box[2] + box[1] * box[2]))) + box_c, 1)
    r_cyl, h_cyl = 0.04, 0.12
    cyl_c = np.array([box_c[0] + box[0] / 2 + 0.03 + r_cyl, 0.0, table_z + h_cyl / 2])
    add(_cylinder_surface(rng, r_cyl, h_cyl, int(density * (2 * np.pi * r_cyl * h_cyl + np.pi * r_cyl ** 2))) + cyl_c, 2)
    r_cap = 0.05
    add(_sphere_cap(rng, r_cap, int(density * 2 * np.pi * r_cap ** 2)) + np.array([-0.40, 0.05, table_z]), 3)
    box2 = (0.05, 0.12, 0.07)
    add(_box_surface(rng, box2, int(density * 2 * (box2[0] * box2[1] + box2[0] * box2[2] + box2[1] * box2[2])))
        + np.array([0.0, 0.42, table_z + box2[2] / 2]), 4)
    strip = np.stack([rng.uniform(-0.45, 0.45, 1200), rng.uniform(-0.003, 0.003, 1200), np.full(1200, table_z)], axis=1)
    add(strip + np.array([0.0, -0.40, 0.0]), 5)
    for k, (c, m) in enumerate([((-0.30, -0.22), 40), ((0.30, -0.25), 120), ((-0.25, 0.35), 250), ((0.35, 0.35), 90),
                                ((-0.55, -0.10), 180)]):
        add(rng.normal(0.0, 0.006, (m, 3)) + np.array([c[0], c[1], table_z + 0.01]), 6 + k)
    pts = np.concatenate(parts).astype(np.float32)
    oid = np.concatenate(ids)
    order = rng.permutation(len(pts))
    return pts[order], oid[order]


def tabletop_camera_pose():
    """(R, t): scene coordinates of tabletop_objects() -> the camera frame of tabletop_frame() (camera at the origin looking
    along +z, the table tilted 35 degrees against the optical axis and rolled 7 degrees: its normal has no zero component)."""
    th = np.deg2rad(35.0)
    tilt = np.array([[1.0, 0.0, 0.0], [0.0, -np.sin(th), -np.cos(th)], [0.0, np.cos(th), -np.sin(th)]])
    return rot_xyz(0.0, 0.0, 7.0) @ tilt, np.array([0.05, 0.30, 1.60])


def tabletop_frame(n: int = 307200, seed: int = 31):
    """A whole cropped camera frame of n points, as a sensor in front of a table would see it: the table top (a 1.5 m x 1.2 m
    rectangle, the largest plane by far), the objects of tabletop_objects() standing on it (thinned for small n), floor 0.7 m
    below and a low wall behind, both only OUTSIDE the table's rectangle, range noise of 1 mm along the viewing ray, 2 % NaN points;
    shuffled.  Two sizes are used: n = 20000 for host-side reference runs, n = 307200 (640 x 480) for the device.
    Returns (points float32 (n, 3), label int32 (n,)): 0-10 the object ids of tabletop_objects(), 100 table, 101 floor, 102 wall,
    -1 a NaN point."""
    rng = np.random.default_rng(seed)
    small = n < 100000
    obj, oid = tabletop_objects(n_drill=1500, density=8000.0, seed=seed + 1) if small else tabletop_objects(seed=seed + 1)
    if len(obj) > n // 3:
        raise ValueError("tabletop_frame: n is too small for the objects")
    n_nan = n // 50
    n_rest = n - len(obj) - n_nan
    n_table, n_floor = int(n_rest * 0.62), int(n_rest * 0.22)
    n_wall = n_rest - n_table - n_floor
    table_z = GT_T[2] - 0.12
    half = np.array([0.75, 0.60])
    table = np.concatenate([rng.uniform(-half, half, (n_table, 2)), np.full((n_table, 1), table_z)], axis=1)
    # floor: a 3.2 m x 2.8 m sheet 0.7 m below the table, minus the table's rectangle (with 5 cm to spare)
    floor = np.zeros((0, 2))
    while len(floor) < n_floor:
        c = rng.uniform([-1.6, -1.4], [1.6, 1.4], (2 * n_floor, 2))
        floor = np.concatenate([floor, c[(np.abs(c) > half + 0.05).any(axis=1)]])
    floor = np.concatenate([floor[:n_floor], np.full((n_floor, 1), table_z - 0.7)], axis=1)
    # wall: upright, 0.8 m behind the table's far edge, ending 5 cm below the table top (nothing but the table lies in its plane)
    wall = np.stack([rng.uniform(-1.6, 1.6, n_wall), np.full(n_wall, half[1] + 0.8), rng.uniform(table_z - 0.7, table_z - 0.05, n_wall)], axis=1)
    pts = np.concatenate([obj.astype(np.float64), table, floor, wall])
    lab = np.concatenate([oid, np.full(n_table, 100, np.int32), np.full(n_floor, 101, np.int32), np.full(n_wall, 102, np.int32)])
    R, t = tabletop_camera_pose()
    cam = pts @ R.T + t
    rng_len = np.linalg.norm(cam, axis=1, keepdims=True)
    cam = cam * (1.0 + rng.normal(0.0, 0.001, (len(cam), 1)) / rng_len)
    cam = np.concatenate([cam, np.full((n_nan, 3), np.nan)])
    lab = np.concatenate([lab, np.full(n_nan, -1, np.int32)])
    order = rng.permutation(n)
    return cam[order].astype(np.float32), lab[order].astype(np.int32)


TABLETOP_DEPTH_CAMERA_SHIFT = np.array([0.0, 0.22, 0.40])


def tabletop_depth_image(rows: int = 480, cols: int = 640, seed: int = 31, drill_shift=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The scene of tabletop_frame() as the sensor's 16-bit depth image (millimetres, holes 0): its rows * cols points seen
    from TABLETOP_DEPTH_CAMERA_SHIFT (0.40 m closer, 0.22 m lower) off tabletop_camera_pose() (the table then lies inside the Kinect preset's 2 m and
    around its swapped principal point), rendered through that preset by depth.render_depth.  The floor lies beyond 2 m and
    drops out in the conversion.  drill_shift moves the model ("drill") by that much in the scene's coordinates (along the table:
    x, y), for the later frames of a sequence."""
    from .depth import preset_params, render_depth
    pts, lab = tabletop_frame(rows * cols, seed)
    pts = pts.astype(np.float64)
    pts[lab == 0] += tabletop_camera_pose()[0] @ np.asarray(drill_shift, np.float64)
    return render_depth(pts - TABLETOP_DEPTH_CAMERA_SHIFT, preset_params("kinect"), rows, cols)
