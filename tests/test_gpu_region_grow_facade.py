"""SegmentationRegionGrow end to end: the C++ façade through region_grow_check against Context.region_grow on the device
(clusters, colours, the return value, and the reference's own sequence of PassThrough, NormalEstimation and RegionGrowing), and
the driver's --frame ... --region-grow down to a pose."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

pcd = importlib.import_module("object-pose-estimation_amd.pcd")
BUILD = os.path.join(ROOT, "object-pose-estimation_amd", "build")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    c = load_pkg().Context(0)
    yield c
    c.close()


def fnv(data: bytes) -> str:
    """FNV-1a (64 bit), as include/ope/region_grow_check.cpp prints it"""
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def _lines(out, prefix):
    return [ln for ln in out.splitlines() if ln.startswith(prefix)]


@pytest.fixture(scope="module")
def frame():
    """The decimated drill model standing free above a curved support (a sector of a cylinder of radius 0.6 m, no plane fits it),
    300 points beyond the z crop and five NaN rows among them; the model; what the crop over z in [0, 1.2] keeps."""
    rng = np.random.default_rng(31)
    model, _ = pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))
    model = np.ascontiguousarray(model, np.float32)
    a, b = rng.uniform(-0.35, 0.35, 3000), rng.uniform(-0.3, 0.3, 3000)
    support = np.column_stack([b, 0.1 + 0.6 * (1 - np.cos(a)), 0.85 + 0.6 * np.sin(a)])   # its axis along x, 4 cm from the drill
    drill = model.astype(np.float64) + np.array([0.0, -0.05, 0.8])
    far = np.column_stack([rng.uniform(-0.3, 0.3, 300), rng.uniform(-0.3, 0.3, 300), rng.uniform(1.25, 1.6, 300)])
    bad = np.full((5, 3), np.nan)
    pts = np.concatenate([drill, support + rng.normal(0, 2e-4, support.shape), far, bad]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero((pts[:, 2] >= 0.0) & (pts[:, 2] <= 1.2) & np.isfinite(pts).all(axis=1)).astype(np.int32)
    assert len(keep) == len(model) + 3000
    return pts, model, keep


def test_facade_region_grow_equals_the_python_path(ctx, frame, tmp_path):
    pts, model, keep = frame
    path = str(tmp_path / "frame.pcd")
    rgb = np.arange(len(pts), dtype=np.uint32)   # the colour of a point is its index in the frame
    pcd.write_pcd(path, pts, rgb=rgb)
    r = subprocess.run([os.path.join(BUILD, "region_grow_check"), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    crop = pts[keep]
    clusters, labels, stats = ctx.region_grow(ctx.upload(crop))
    assert len(clusters) >= 2 and min(len(c) for c in clusters) >= 500
    assert _lines(r.stdout, "crop ") == ["crop %d" % len(keep)]
    assert _lines(r.stdout, "regions ") == ["regions %d sweeps %d one_way %d" % (len(clusters), stats["sweeps"], stats["one_way_edges"])]
    assert _lines(r.stdout, "region ") == ["region %d %d %s %s" % (k, len(c), fnv(crop[c].tobytes()), fnv(rgb[keep[c]].tobytes()))
                                          for k, c in enumerate(clusters)]
    assert _lines(r.stdout, "last ") == ["last %d %s" % (len(clusters[-1]), fnv(crop[clusters[-1]].tobytes()))]
    # the reference's own sequence of classes gives the same clusters (normals passed in equal normals estimated by the call)
    assert _lines(r.stdout, "classes ") == ["classes %d" % len(clusters)]
    assert _lines(r.stdout, "class ") == ["class %d %d %s" % (k, len(c), fnv(crop[c].tobytes())) for k, c in enumerate(clusters)]


def test_driver_region_grow_reaches_a_pose(ctx, frame, tmp_path):
    pts, model, keep = frame
    exe = os.path.join(BUILD, "detect_and_localize")
    mp, fp = str(tmp_path / "model.pcd"), str(tmp_path / "frame.pcd")
    pcd.write_pcd(mp, model)
    pcd.write_pcd(fp, pts)
    clusters, _, stats = ctx.region_grow(ctx.upload(pts[keep]))
    a = subprocess.run([exe, "--frame", mp, fp, "--region-grow", "--seed", "1"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0, a.stdout + a.stderr
    print(a.stdout)
    assert _lines(a.stdout, "segment crop ") == ["segment crop %d sweeps %d" % (len(keep), stats["sweeps"])]
    assert _lines(a.stdout, "segment clusters ") == ["segment clusters %d sizes %s" % (len(clusters), " ".join(str(len(c)) for c in clusters))]
    assert _lines(a.stdout, "candidates ") == ["candidates selected %s clusters %d" % (_lines(a.stdout, "candidates ")[0].split()[2], len(clusters))]
    pose = _lines(a.stdout, "frame 1 ")
    assert len(pose) == 1 and "final" in pose[0]
    vals = [float(v) for v in pose[0].split("final")[1].split("coarse")[0].split()]
    assert len(vals) == 16 and all(math.isfinite(v) for v in vals)
    # the flag is refused without --frame
    b = subprocess.run([exe, mp, fp, "--region-grow"], capture_output=True, text=True, timeout=60)
    assert b.returncode == 2
