"""The scenes of the peel tests (not a test module): a room-like frame without a single table.  Three noisy planar patches that do
not touch (floor y = 0.25, back wall z = 1.55, side wall x = 0.47; +-3 mm), four blobs (1500, 1200, 900 and 250 points: cubes of
half-edge 40, 38, 35 and 20 mm) well away from the planes, the rest uniform noise; float32, shuffled by a seeded permutation."""
import numpy as np

BLOBS = ((1500, 0.040, (-0.25, 0.00, 0.90)), (1200, 0.038, (0.10, -0.20, 1.10)), (900, 0.035, (0.20, 0.05, 0.80)),
         (250, 0.020, (-0.15, -0.30, 1.30)))


def room_scene(sizes=(8000, 5000, 3000), n=20000, seed=1, scale=1.0):
    """sizes: the points of floor, back wall and side wall.  scale multiplies every count: the same make-up with more or fewer
    points (15.36: a 307 200-point frame)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform
    nf, nb, ns = (int(round(s * scale)) for s in sizes)
    n = int(round(n * scale))
    parts = [np.column_stack([u(-0.45, 0.45, nf), 0.25 + u(-0.003, 0.003, nf), u(0.6, 1.5, nf)]),
             np.column_stack([u(-0.45, 0.45, nb), u(-0.45, 0.15, nb), 1.55 + u(-0.003, 0.003, nb)]),
             np.column_stack([0.47 + u(-0.003, 0.003, ns), u(-0.45, 0.15, ns), u(0.6, 1.45, ns)])]
    for k, h, c in BLOBS:
        parts.append(np.asarray(c) + u(-h, h, (int(round(k * scale)), 3)))
    left = n - sum(len(p) for p in parts)
    assert left >= 0
    parts.append(np.column_stack([u(-0.4, 0.4, left), u(-0.4, 0.2, left), u(0.65, 1.5, left)]))
    pts = np.concatenate(parts).astype(np.float32)
    return pts[rng.permutation(n)]


SCENES = {"three": (8000, 5000, 3000), "exact": (8000, 6000, 2000), "over": (8000, 5999, 2000)}


def noise_with_nans(n=3000, seed=4):
    """n uniform points in a 0.5 m cube, seven rows of them NaN."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, 0.5, (n, 3)).astype(np.float32) + np.float32([0, 0, 0.8])
    bad = rng.choice(n, 7, replace=False)
    pts[bad] = np.nan
    return pts, np.sort(bad)
