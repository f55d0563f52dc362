"""Clusters cut on the device go straight into the pose stages: ope_euclidean_clusters_cloud -> ope_final_pose_batch /
ope_track_gate is byte-identical to the same stages on the clusters uploaded from the host, and detect_and_localize --segment
(getClusters through the façade) gives the reference's clusters and the same candidate lines as --candidates on them."""
import dataclasses
import importlib
import os
import subprocess

import numpy as np
import pytest

from cluster_ref import reference_clusters
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

synth = importlib.import_module("object-pose-estimation_amd.synth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "object-pose-estimation_amd", "build", "detect_and_localize")


@pytest.fixture(scope="module")
def ctx():
    c = load_pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model():
    xyz, _ = pcd.read_pcd(os.path.join(GOLD, "drill_model_decimated.pcd"))
    return np.ascontiguousarray(xyz, np.float32)


@pytest.fixture(scope="module")
def scene():
    return synth.tabletop_objects()[0]


def _bytes(v):
    if dataclasses.is_dataclass(v):
        return b"".join(_bytes(getattr(v, f.name)) for f in dataclasses.fields(v))
    if isinstance(v, np.ndarray):
        return v.tobytes()
    if isinstance(v, (list, tuple)):
        return b"".join(_bytes(x) for x in v)
    if isinstance(v, float):
        return v.hex().encode()
    return repr(v).encode()


def test_cloud_form_is_what_select_builds(ctx, scene):
    ope = load_pkg()
    cloud = ctx.upload(scene, normals=np.tile(np.array([0, 0, 1], np.float32), (len(scene), 1)) + scene * 0.5)
    clouds, idx = ctx.euclidean_clusters_cloud(cloud)
    want = reference_clusters(scene, 0.05, 300, 100000)
    assert [c.tolist() for c in idx] == [c.tolist() for c in want]
    for c, i in zip(clouds, idx):
        sel = ctx.select(cloud, i)
        a = np.empty((c.n, 3), np.float32)
        b = np.empty((sel.n, 3), np.float32)
        ctx._chk(ope.lib().ope_cloud_download(ctx.h, c.h, a.ctypes.data_as(ope._fp)))
        ctx._chk(ope.lib().ope_cloud_download(ctx.h, sel.h, b.ctypes.data_as(ope._fp)))
        assert a.tobytes() == b.tobytes() == scene[i].tobytes()
    s = ctx.cluster_stats()
    assert s["host_syncs"] == 2


def test_final_pose_batch_on_device_clusters_equals_host_upload(ctx, model, scene):
    m = ctx.upload(model)
    dev, idx = ctx.euclidean_clusters_cloud(scene)
    host = [ctx.upload(scene[i]) for i in idx]
    a, sa = ctx.final_pose_batch(m, dev)
    b, sb = ctx.final_pose_batch(m, host)
    assert sa == sb
    assert _bytes(a) == _bytes(b)
    ga = ctx.track_gate(m, dev)
    gb = ctx.track_gate(m, host)
    assert _bytes(ga) == _bytes(gb)


def _lines(out, prefix):
    return [ln for ln in out.splitlines() if ln.startswith(prefix)]


def test_driver_segment_matches_candidates_on_the_same_clusters(tmp_path, model, scene):
    mp, sp = str(tmp_path / "model.pcd"), str(tmp_path / "not_plane.pcd")
    pcd.write_pcd(mp, model)
    pcd.write_pcd(sp, scene)
    r = subprocess.run([EXE, "--segment", mp, sp, "--seed", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    seg = _lines(r.stdout, "segment clusters ")
    want = reference_clusters(scene, 0.05, 300, 100000)
    assert seg == ["segment clusters %d sizes %s" % (len(want), " ".join(str(len(c)) for c in want))]
    paths = []
    for k, c in enumerate(want):
        paths.append(str(tmp_path / ("cluster%d.pcd" % k)))
        pcd.write_pcd(paths[-1], scene[c])
    r2 = subprocess.run([EXE, mp, *paths, "--seed", "1", "--candidates"], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    for prefix in ("candidates ", "frame "):
        assert _lines(r.stdout, prefix) == _lines(r2.stdout, prefix) and _lines(r.stdout, prefix)
