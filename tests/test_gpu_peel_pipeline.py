"""getSegmentedObjectsExceptPlane end to end: Context.except_plane_segment against tests/peel_ref.py (exact), the C++ façade
through segmentation_check --except-plane against the Python path on the device (clusters and colours), and the driver's
--frame ... --except-plane against --segment on the same remainder."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import peel_ref as pf
from conftest import ROOT, load_pkg
from peel_scenes import SCENES, room_scene

pytestmark = pytest.mark.gpu

pcd = importlib.import_module("object-pose-estimation_amd.pcd")
BUILD = os.path.join(ROOT, "object-pose-estimation_amd", "build")
GOLD = os.path.join(ROOT, "tests", "golden")
LO, HI = np.float32([-0.5, -0.5, 0.5]), np.float32([0.5, 0.3, 1.6])   # getFiltered's literals (objectsegmentationplane.cpp:17)


@pytest.fixture(scope="module")
def ctx():
    c = load_pkg().Context(0)
    yield c
    c.close()


def fnv(data: bytes) -> str:
    """FNV-1a (64 bit), as include/ope/segmentation_check.cpp prints it"""
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def _lines(out, prefix):
    return [ln for ln in out.splitlines() if ln.startswith(prefix)]


@pytest.fixture(scope="module")
def frame():
    """the three-plane room with 600 points outside getFiltered's box and five NaN rows among it; what the crop keeps; the
    reference's clusters of that (as indices of the crop) and its peel"""
    rng = np.random.default_rng(21)
    room = room_scene(SCENES["three"])
    far = np.column_stack([rng.uniform(-0.4, 0.4, 600), rng.uniform(-0.4, 0.2, 600), rng.uniform(1.7, 2.0, 600)]).astype(np.float32)
    bad = np.full((5, 3), np.nan, np.float32)
    pts = np.concatenate([room, far, bad])[rng.permutation(len(room) + 605)]
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero(((pts >= LO) & (pts <= HI)).all(axis=1)).astype(np.int32)
    assert len(keep) == 20000
    clusters, peel = pf.except_plane(pts[keep], seed=12345)
    assert sorted(peel["counts"].tolist()) == [3000, 5000, 8000] and len(peel["rest_idx"]) == 4000 and len(clusters) == 3
    return pts, keep, clusters, peel


@pytest.mark.parametrize("name,max_planes", [("three", 0), ("exact", 0), ("exact", 1)])
def test_except_plane_segment_equals_the_reference(ctx, name, max_planes):
    ope = load_pkg()
    pts = room_scene(SCENES[name])
    want, wp = pf.except_plane(pts, max_planes=max_planes, seed=2)
    first = {("three", 0): (3, None), ("exact", 0): (4, 2000), ("exact", 1): (5, 6000)}[(name, max_planes)]   # clusters, the largest
    assert len(want) == first[0] and (first[1] is None or len(want[0]) == first[1])
    clouds, got, peel = ctx.except_plane_segment(ctx.upload(pts), ope.default_plane_params(seed=2), max_planes=max_planes, want_clouds=True)
    print("[except-plane] %s planes %s rest %d clusters %s" % (name, peel.counts.tolist(), len(peel.rest_idx), [len(c) for c in got]))
    assert peel.stop == wp["stop"] and np.array_equal(peel.counts, wp["counts"]) and np.array_equal(peel.rest_idx, wp["rest_idx"])
    assert [c.tolist() for c in got] == [c.tolist() for c in want]
    for cloud, idx in zip(clouds, want):
        assert ctx.download(cloud).tobytes() == pts[idx].tobytes()
    only, _ = ctx.except_plane_segment(ctx.upload(pts), ope.default_plane_params(seed=2), max_planes=max_planes)
    assert [c.tolist() for c in only] == [c.tolist() for c in want]


def test_facade_except_plane_equals_the_python_path(ctx, frame, tmp_path):
    pts, keep, want, wp = frame
    path = str(tmp_path / "frame.pcd")
    rgb = np.arange(len(pts), dtype=np.uint32)   # the colour of a point is its index in the frame
    pcd.write_pcd(path, pts, rgb=rgb)
    r = subprocess.run([os.path.join(BUILD, "segmentation_check"), path, "--except-plane"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    crop = pts[keep]
    clusters, peel = ctx.except_plane_segment(ctx.upload(crop))
    assert [c.tolist() for c in clusters] == [c.tolist() for c in want]
    assert _lines(r.stdout, "filtered ") == ["filtered %d %s" % (len(keep), fnv(crop.tobytes()))]
    assert _lines(r.stdout, "except planes ") == ["except planes %d sizes %s rest %d clusters %d" % (
        len(peel.counts), " ".join(str(c) for c in peel.counts), len(peel.rest_idx), len(clusters))]
    assert _lines(r.stdout, "except cluster ") == ["except cluster %d %d %s %s" % (k, len(c), fnv(crop[c].tobytes()), fnv(rgb[keep[c]].tobytes()))
                                                  for k, c in enumerate(clusters)]
    # without the flag the program prints what it printed before
    q = subprocess.run([os.path.join(BUILD, "segmentation_check"), path], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0 and q.stdout and r.stdout.startswith(q.stdout) and "except" not in q.stdout and "filtered" not in q.stdout


def test_driver_except_plane_ends_on_the_pose_of_segment_on_the_same_remainder(ctx, frame, tmp_path):
    pts, keep, want, wp = frame
    model, _ = pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))
    exe = os.path.join(BUILD, "detect_and_localize")
    mp, fp, sp = str(tmp_path / "model.pcd"), str(tmp_path / "frame.pcd"), str(tmp_path / "rest.pcd")
    pcd.write_pcd(mp, np.ascontiguousarray(model, np.float32))
    pcd.write_pcd(fp, pts)
    crop = pts[keep]
    _, peel = ctx.except_plane_segment(ctx.upload(crop))
    assert np.array_equal(peel.rest_idx, wp["rest_idx"])
    pcd.write_pcd(sp, crop[peel.rest_idx])
    limits = [str(float(v)) for v in (LO[0], HI[0], LO[1], HI[1], LO[2], HI[2])]
    a = subprocess.run([exe, "--frame", mp, fp, "--except-plane", "--limits", *limits, "--seed", "1"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0, a.stdout + a.stderr
    b = subprocess.run([exe, "--segment", mp, sp, "--seed", "1"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    print(a.stdout)
    assert _lines(a.stdout, "segment planes ") == ["segment planes %d sizes %s rest %d" % (len(peel.counts), " ".join(str(c) for c in peel.counts),
                                                                                          len(peel.rest_idx))]
    assert _lines(a.stdout, "segment clusters ") == ["segment clusters 3 sizes " + " ".join(str(len(c)) for c in want)]
    for prefix in ("segment clusters ", "candidates ", "frame "):
        assert _lines(a.stdout, prefix) == _lines(b.stdout, prefix) and _lines(a.stdout, prefix)
    # without the flag nothing changes: --frame still runs the table-top segmentation
    assert not _lines(a.stdout, "segment plane ")
