"""BuildModel from the sensor's images: buildmodel.build_model_from_images (coloured ingest with the crop, table, cluster 0 and
the sequential registration, all on device clouds) against register_point_clouds fed with the same clusters fetched to the
host, byte for byte; and the build_model --scan program on the same images written to files, whose .pcd holds the same points
and colours."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import scan_scene as ss
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

buildmodel = importlib.import_module("object-pose-estimation_amd.buildmodel")
depth_mod = importlib.import_module("object-pose-estimation_amd.depth")
pcd = importlib.import_module("object-pose-estimation_amd.pcd")
# a threshold that is the same number as a float and as a double: the program parses it into a float
KW = dict(corr_rej_thresh=0.75, max_iterations=10)


@pytest.fixture(scope="module")
def env():
    ope = load_pkg()
    ctx = ope.Context(0)
    yield ope, ctx
    ctx.close()


@pytest.fixture(scope="module")
def scan(env):
    ope, ctx = env
    pairs = ss.image_pairs()
    par = ope.default_depth_params(ss.SENSOR)
    res = buildmodel.build_model_from_images(ope, ctx, [d for d, _ in pairs], [c for _, c in pairs], ss.LIMITS, params=par, **KW)
    return pairs, par, res


def test_model_from_images_equals_the_registration_of_the_fetched_clusters(env, scan):
    ope, ctx = env
    pairs, par, res = scan
    lim = np.asarray(ss.LIMITS, np.float32).reshape(3, 2)
    xyz, rgb = [], []
    for d, c in pairs:
        frame = ctx.depth_to_cloud(d, par, lim[:, 0], lim[:, 1], bgr=c)
        obj = buildmodel.segment_object_device(ope, ctx, frame)
        assert obj.has_rgb and 300 <= obj.n < 5000 and frame.n < 10000
        xyz.append(ctx.download(obj))
        rgb.append(obj.download_rgb())
    print("[scan] frames of", [int((d > 0).sum()) for d, _ in pairs], "pixels, clusters of", [len(x) for x in xyz], "points")
    ref = buildmodel.register_point_clouds(ope, ctx, xyz, **KW)
    assert len(res.pairs) == len(ref.pairs) == 2
    for a, b in zip(res.pairs, ref.pairs):
        assert np.asarray(a.T).tobytes() == np.asarray(b.T).tobytes() and a.iterations == b.iterations <= 10
    assert res.cloud.tobytes() == ref.cloud.tobytes()
    assert res.rgb.dtype == np.uint32 and np.array_equal(res.rgb, np.concatenate(rgb))
    # every colour is a pixel's colour
    words = {int(w) for _, c in pairs for w in (c[..., 2].astype(np.uint32) << 16 | c[..., 1].astype(np.uint32) << 8 | c[..., 0]).reshape(-1)}
    assert set(res.rgb.tolist()) <= words


def test_a_frame_without_a_table_is_refused(env):
    ope, ctx = env
    d = np.zeros((ss.ROWS, ss.COLS), np.uint16)
    c = np.zeros((ss.ROWS, ss.COLS, 3), np.uint8)
    with pytest.raises(ValueError, match="frame 0"):
        buildmodel.build_model_from_images(ope, ctx, [d], [c], ss.LIMITS, params=ope.default_depth_params(ss.SENSOR), **KW)


def test_scan_program_writes_the_same_model(env, scan, tmp_path):
    pairs, _, res = scan
    exe = os.path.join(ROOT, "object-pose-estimation_amd", "build", "build_model")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    files = []
    for i, (d, c) in enumerate(pairs):
        files += [str(tmp_path / ("depth%d.pgm" % i)), str(tmp_path / ("rgb%d.ppm" % i))]
        depth_mod.write_pgm16(files[-2], d)
        depth_mod.write_ppm8(files[-1], c)
        assert np.array_equal(depth_mod.read_ppm8(files[-1]), c)
    out = str(tmp_path / "model.pcd")
    r = subprocess.run([exe, "--scan", ss.SENSOR, "--limits", *["%r" % float(v) for v in ss.LIMITS], out, "0.75", "10", *files],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Finished segmentation of 3 point clouds!" in r.stdout and r.stdout.count("\npair ") == 2
    xyz, rgb = pcd.read_pcd(out)
    assert xyz.tobytes() == res.cloud.tobytes()
    assert np.array_equal(rgb, res.rgb)
    # a frame without a table: a message and status 5
    depth_mod.write_pgm16(files[0], np.zeros((ss.ROWS, ss.COLS), np.uint16))
    r = subprocess.run([exe, "--scan", ss.SENSOR, "--limits", *["%r" % float(v) for v in ss.LIMITS], out, "0.75", "10", *files[:2]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 5 and "no supporting plane" in r.stderr


# ---------------------------------------------------------------- the façade's host clouds of a coloured device frame
SEGMENT = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ope/data_grabber.hpp"
#include "ope/object_segmentation_plane.hpp"
static void show(const char *tag, const ope::ObjectSegmentationPlane::Cloud &c) {
  unsigned long long hx = 1469598103934665603ull, hc = hx;
  for (const auto &p : c.points) {
    unsigned char b[16];
    std::memcpy(b, &p.x, 12);
    std::memcpy(b + 12, &p.rgb, 4);
    for (int i = 0; i < 12; ++i) hx = (hx ^ b[i]) * 1099511628211ull;
    for (int i = 12; i < 16; ++i) hc = (hc ^ b[i]) * 1099511628211ull;
  }
  std::printf("%s %zu xyz %016llx rgb %016llx\n", tag, c.size(), hx, hc);
}
int main(int argc, char **argv) {
  ope::DepthImage depth;
  ope::ColorImage colour;
  if (ope::io::loadPGM(argv[1], depth) != 0 || ope::io::loadPPM(argv[2], colour) != 0) return 3;
  float lo[3], hi[3];
  for (int d = 0; d < 3; ++d) { lo[d] = std::strtof(argv[3 + 2 * d], nullptr); hi[d] = std::strtof(argv[4 + 2 * d], nullptr); }
  ope::DataGrabber grabber(true, false, false);
  auto frame = grabber.rgbd2PclDevice(colour, depth, lo, hi);
  if (!frame->h) return 6;
  ope::ObjectSegmentationPlane seg;
  std::vector<ope::ObjectSegmentationPlane::Cloud::Ptr> clusters;
  ope::ObjectSegmentationPlane::Cloud::Ptr plane;
  const bool isPlane = seg.getSegmentedObjectsOnPlane(*frame, clusters, plane);
  std::printf("plane %d clusters %zu device %zu\n", (int)isPlane, clusters.size(), isPlane ? seg.deviceClusters().size() : (size_t)0);
  show("plane", *plane);
  for (const auto &c : clusters) show("cluster", *c);
  for (size_t k = 0; isPlane && k < seg.deviceClusters().size(); ++k) std::printf("coloured %d\n", ope_cloud_has_rgb(seg.deviceClusters()[k]->h));
  return 0;
}
'''


def _fnv(b) -> str:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_facade_host_clouds_of_a_coloured_device_frame(env, tmp_path):
    """ObjectSegmentationPlane::getSegmentedObjectsOnPlane on a coloured rgbd2PclDevice frame: the host plane and clusters hold the
    points of the device clouds and the colours of `bgr` gathered through the pixels (one ope_cloud_download_rgb per cloud); a
    frame without a plane comes back as cluster 0 with its own colours."""
    ope, ctx = env
    LIB = os.path.join(ROOT, "object-pose-estimation_amd")
    src, exe = tmp_path / "segment.cpp", str(tmp_path / "segment")
    src.write_text(SEGMENT)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", LIB, "-lope_hip",
                           "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"])
    d, c = ss.image_pairs(1)[0]
    lonely = np.zeros_like(d)
    lonely[60, 80], lonely[61, 85] = 800, 900          # two points: no plane, the frame is handed back
    par = ope.default_depth_params(ss.SENSOR)
    lim = np.asarray(ss.LIMITS, np.float32).reshape(3, 2)
    flat = c.reshape(-1, 3).astype(np.uint32)
    word = flat[:, 2] << 16 | flat[:, 1] << 8 | flat[:, 0]
    for name, img in (("scene", d), ("lonely", lonely)):
        dp, cp = str(tmp_path / (name + ".pgm")), str(tmp_path / (name + ".ppm"))
        depth_mod.write_pgm16(dp, img)
        depth_mod.write_ppm8(cp, c)
        r = subprocess.run([exe, dp, cp, *["%r" % float(v) for v in ss.LIMITS]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        frame, pix = ctx.depth_to_cloud(img, par, lim[:, 0], lim[:, 1], want_pixels=True, bgr=c)
        seg = ctx.tabletop_segment(frame)
        line = lambda tag, xyz, rgb: "%s %d xyz %s rgb %s" % (tag, len(xyz), _fnv(np.ascontiguousarray(xyz, np.float32).tobytes()), _fnv(rgb.astype("<u4").tobytes()))
        if name == "lonely":
            assert seg.status != ope.TABLETOP_OK and frame.n == 2
            assert lines == ["plane 0 clusters 1 device 0", "plane 0 xyz %s rgb %s" % (_fnv(b""), _fnv(b"")),
                             line("cluster", ctx.download(frame), word[pix])]
            continue
        assert seg.status == ope.TABLETOP_OK
        clouds, idx = ctx.euclidean_clusters_cloud(seg.not_plane)
        assert len(clouds) >= 1
        want = ["plane 1 clusters %d device %d" % (len(clouds), len(clouds)), line("plane", ctx.download(seg.plane), word[pix[seg.plane_idx]])]
        want += [line("cluster", ctx.download(k), word[pix[seg.not_plane_idx][i]]) for k, i in zip(clouds, idx)]
        want += ["coloured 1"] * len(clouds)
        assert lines == want
